"""numpy / scipy restatement of the multigrid cycles with a Chebyshev polynomial smoother, for the tests.

The cycles follow the device driver (which follows amg_matrix.cpp:160-378): V, W and BS, ProxySmoother composition (sm_steps,
sm_symm) and the flag contract of base_smoother.hpp:68-112.  Per level the smoother is

    "jacobi"  x += omega Dinv r                                  (the oracle's RichardsonSmoother; ties this file to the oracle)
    "cheby"   degree k on [lmax / ratio, lmax]:
              theta = (lmax+lmin)/2, delta = (lmax-lmin)/2, sigma = theta/delta, rho_1 = 1/sigma
              step 1:        d = (1/theta) Dinv r,  x += d
              step j = 2..k: rho_j = 1/(2 sigma - rho_{j-1}),  d = rho_j rho_{j-1} d + (2 rho_j/delta) Dinv (b - A x),  x += d
    callable  smooth(level, x, b, res, res_updated, update_res, x_zero, back) working in place (e.g. Oracle.smooth for
              Gauss-Seidel levels of a mixed hierarchy)

with r = b when x_zero and not res_updated, r = res when res_updated, r = b - A x otherwise; update_res forms res = b - A x at
the end.  Levels come from Hierarchy.levels (A, P, PT, dinv, free)."""
import numpy as np


def cheby_coefficients(lmax, ratio, degree):
    lmin = lmax / ratio
    theta, delta = 0.5 * (lmax + lmin), 0.5 * (lmax - lmin)
    sigma = theta / delta
    rho = 1.0 / sigma
    c1, c2 = [0.0, 0.0], [0.0, 0.0]          # index = step j (entries 0, 1 unused)
    for _ in range(2, degree + 1):
        rn = 1.0 / (2.0 * sigma - rho)
        c1.append(rn * rho)
        c2.append(2.0 * rn / delta)
        rho = rn
    return 1.0 / theta, c1, c2


class LevelOps:
    def __init__(self, lv):
        self.A = lv.A.to_scipy()
        self.P = lv.P.to_scipy() if lv.P is not None else None
        self.PT = lv.PT.to_scipy() if lv.PT is not None else None
        self.bs = lv.A.br
        self.n = lv.A.n_rows * self.bs
        self.dinv = np.asarray(lv.dinv, dtype=np.float64).reshape(lv.A.n_rows, self.bs, self.bs).copy()

    def D(self, v):
        if self.bs == 1:
            return self.dinv[:, 0, 0] * v
        return np.einsum("nij,nj->ni", self.dinv, v.reshape(-1, self.bs)).reshape(-1)


def fill_vector(n, seed):
    """the device's deterministic pseudo-random vector (fill_kernel): splitmix64 of i * golden + seed, mapped to [-1, 1)"""
    with np.errstate(over="ignore"):
        z = np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(seed)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(11)).astype(np.float64) * (2.0 / 9007199254740992.0) - 1.0


def power_estimate(lv, steps=30, v0=None):
    """the estimator of amgx_create restated: v_0 = Dinv A f (f = fill_vector(n, 1)); per step t = A v, w = Dinv t,
    lambda = <t, w> / <t, v>, v <- w / lambda.  Returns the last lambda (a lower bound of lambda_max(Dinv A) for symmetric
    positive semi-definite A and Dinv)."""
    ops = lv if isinstance(lv, LevelOps) else LevelOps(lv)
    f = fill_vector(ops.n, 1) if v0 is None else v0
    v = ops.D(ops.A @ f)
    lam = 0.0
    for _ in range(steps):
        t = ops.A @ v
        w = ops.D(t)
        num, den = float(t @ w), float(t @ v)
        if not (num > 0.0 and den > 0.0):
            break
        lam = num / den
        v = w / lam
    return lam


def lambda_true(lv):
    """lambda_max(Dinv A) from a symmetric eigenvalue solve: Dinv = S S with S the blockwise square root of the (pseudo-)inverse
    diagonal blocks, and lambda(Dinv A) = lambda(S A S)"""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla
    ops = lv if isinstance(lv, LevelOps) else LevelOps(lv)
    sym = 0.5 * (ops.dinv + np.transpose(ops.dinv, (0, 2, 1)))
    w, q = np.linalg.eigh(sym)
    s = np.einsum("nij,nj,nkj->nik", q, np.sqrt(np.maximum(w, 0.0)), q)
    nb = s.shape[0]
    S = sp.bsr_matrix((s, np.arange(nb), np.arange(nb + 1)), shape=(ops.n, ops.n)).tocsr() if ops.bs > 1 else sp.diags(s[:, 0, 0])
    M = (S @ ops.A @ S).tocsr()
    M = 0.5 * (M + M.T)
    if ops.n <= 400:
        return float(np.linalg.eigvalsh(M.toarray())[-1])
    return float(spla.eigsh(M, k=1, which="LA", tol=1e-13, ncv=40, maxiter=200000, return_eigenvectors=False)[0])


class ChebyRef:
    """sm: per level (or one for all) "jacobi", "cheby" or a callable; lambda_max / degree / ratio: scalars or per-level lists"""

    def __init__(self, hierarchy_or_levels, sm="cheby", degree=2, ratio=10.0, lambda_max=None, omega=0.9, sm_steps=1, sm_symm=False,
                 cycle="V", clev="inv", coarse_inv=None):
        H = hierarchy_or_levels
        levels = H.levels if hasattr(H, "levels") else list(H)
        self.L = len(levels)
        self.ops = [LevelOps(lv) for lv in levels]
        per = lambda v, i: v[i] if isinstance(v, (list, tuple, np.ndarray)) else v
        self.sm = [per(sm, i) for i in range(self.L)]
        self.omega = omega
        self.steps = [int(per(sm_steps, i)) for i in range(self.L)]
        self.symm = [bool(per(sm_symm, i)) for i in range(self.L)]
        self.cycle = cycle
        self.coef = [None] * self.L
        for i in range(self.L - 1):
            if self.sm[i] == "cheby":
                lm = per(lambda_max, i) if lambda_max is not None else None
                if lm is None:
                    lm = 1.1 * power_estimate(self.ops[i])
                self.coef[i] = (int(per(degree, i)),) + cheby_coefficients(float(lm), float(per(ratio, i)), int(per(degree, i)))
        if coarse_inv is None and hasattr(H, "coarse_inv") and clev == "inv":
            n = int(H.coarse_n)
            coarse_inv = np.asarray(H.coarse_inv, dtype=np.float64).reshape(n, n) if n else None
        self.cinv = coarse_inv if clev == "inv" else None
        self.x = [np.zeros(o.n) for o in self.ops]
        self.rhs = [np.zeros(o.n) for o in self.ops]
        self.res = [np.zeros(o.n) for o in self.ops]

    # ---- smoothers: all work in place on x and res ------------------------------------------------------------------
    def base_smooth(self, l, back, x, b, res, ru, ur, xz):
        o, sm = self.ops[l], self.sm[l]
        if callable(sm):
            sm(l, x, b, res, ru, ur, xz, back)
            return
        if sm == "jacobi":
            if not ru and xz:
                x += self.omega * o.D(b)
            else:
                if not ru:
                    res[:] = b - o.A @ x
                x += self.omega * o.D(res)
        else:
            k, c0, c1, c2 = self.coef[l]
            r = b if (xz and not ru) else (res if ru else b - o.A @ x)
            d = c0 * o.D(r)
            if xz:
                x[:] = d
            else:
                x += d
            for j in range(2, k + 1):
                d = c1[j] * d + c2[j] * o.D(b - o.A @ x)
                x += d
        if ur:
            res[:] = b - o.A @ x

    def level_smooth(self, l, back, x, b, res, ru, ur, xz):
        k = max(1, self.steps[l])
        if not self.symm[l] and k == 1:
            self.base_smooth(l, back, x, b, res, ru, ur, xz)
            return
        if self.symm[l]:
            def symm(ru_, xz_):
                self.base_smooth(l, False, x, b, res, ru_, ur, xz_)
                self.base_smooth(l, True, x, b, res, ur, ur, False)
            symm(ru, xz)
            for _ in range(1, k):
                symm(ur, False)
        else:
            self.base_smooth(l, back, x, b, res, ru, ur, xz)
            for _ in range(1, k):
                self.base_smooth(l, back, x, b, res, ur, ur, False)

    def smooth(self, l, x, b, res, res_updated=False, update_res=False, x_zero=False, back=False):
        self.level_smooth(l, back, x, b, res, res_updated, update_res, x_zero)
        return x, res

    # ---- cycles ---------------------------------------------------------------------------------------------------
    def coarse_solve(self, b):
        if self.cinv is None:
            return np.zeros_like(b)
        return self.cinv @ b

    def _pre(self, l, x, b, r):
        x[:] = 0.0
        r[:] = b
        self.level_smooth(l, False, x, b, r, True, True, True)

    def _post(self, l, x, b, r, xc):
        x += self.ops[l].P @ xc
        self.level_smooth(l, True, x, b, r, False, False, False)

    def _v(self, x0, b0):
        L = self.L
        if L == 1:
            x0[:] = self.coarse_solve(b0)
            return
        for l in range(L - 1):
            x, b = (x0, b0) if l == 0 else (self.x[l], self.rhs[l])
            self._pre(l, x, b, self.res[l])
            self.rhs[l + 1][:] = self.ops[l].PT @ self.res[l]
        self.x[L - 1][:] = self.coarse_solve(self.rhs[L - 1])
        for l in range(L - 2, -1, -1):
            x, b = (x0, b0) if l == 0 else (self.x[l], self.rhs[l])
            self._post(l, x, b, self.res[l], self.x[l + 1])

    def _w(self, l, x0, b0):
        L = self.L
        if l + 1 < L:
            x, b = (x0, b0) if l == 0 else (self.x[l], self.rhs[l])
            r = self.res[l]
            self._pre(l, x, b, r)
            self.rhs[l + 1][:] = self.ops[l].PT @ r
            self._w(l + 1, x0, b0)
            x += self.ops[l].P @ self.x[l + 1]
            self.level_smooth(l, True, x, b, r, False, True, False)
            self.level_smooth(l, False, x, b, r, True, True, False)
            self.rhs[l + 1][:] = self.ops[l].PT @ r
            self._w(l + 1, x0, b0)
            self._post(l, x, b, r, self.x[l + 1])
        elif L == 1:
            x0[:] = self.coarse_solve(b0)
        else:
            self.x[L - 1][:] = self.coarse_solve(self.rhs[L - 1])

    def smooth_v_from_level(self, start, x, b, res, ru, ur, xz):
        L = self.L
        self.level_smooth(start, False, x, b, res, ru, True, xz)
        self.rhs[start + 1][:] = self.ops[start].PT @ res
        for l in range(start + 1, L - 1):
            self._pre(l, self.x[l], self.rhs[l], self.res[l])
            self.rhs[l + 1][:] = self.ops[l].PT @ self.res[l]
        self.x[L - 1][:] = self.coarse_solve(self.rhs[L - 1])
        for l in range(L - 2, start, -1):
            self._post(l, self.x[l], self.rhs[l], self.res[l], self.x[l + 1])
        x += self.ops[start].P @ self.x[start + 1]
        self.level_smooth(start, True, x, b, res, False, ur, False)

    def _bs(self, x0, b0):
        L = self.L
        if L == 1:
            x0[:] = self.coarse_solve(b0)
            return
        for l in range(L - 1):
            x, b = (x0, b0) if l == 0 else (self.x[l], self.rhs[l])
            r = self.res[l]
            x[:] = 0.0
            r[:] = b
            self.smooth_v_from_level(l, x, b, r, True, True, True)
            self.rhs[l + 1][:] = self.ops[l].PT @ r
        self.x[L - 1][:] = self.coarse_solve(self.rhs[L - 1])
        for l in range(L - 2, -1, -1):
            x, b = (x0, b0) if l == 0 else (self.x[l], self.rhs[l])
            x += self.ops[l].P @ self.x[l + 1]
            self.smooth_v_from_level(l, x, b, self.res[l], False, False, False)

    def apply(self, b):
        b = np.array(b, dtype=np.float64)
        x = np.zeros_like(b)
        if self.cycle == "W":
            self._w(0, x, b)
        elif self.cycle == "BS":
            self._bs(x, b)
        else:
            self._v(x, b)
        return x

    def pcg(self, b, tol=1e-8, maxit=200, x0=None):
        """CG with this cycle as preconditioner, err_k = sqrt(|<C r_k, r_k>|), stop at err_k <= tol err_0 (the criterion of
        amgx_pcg and of the oracle).  Returns (x, iterations, errs)."""
        A = self.ops[0].A
        x = np.zeros_like(b, dtype=np.float64) if x0 is None else np.array(x0, dtype=np.float64)
        d = b - A @ x
        w = self.apply(d)
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
            w = self.apply(d)
            wd_new = float(w @ d)
            s = w + (wd_new / wd) * s
            wd = wd_new
            errs.append(np.sqrt(abs(wd)))
            if errs[-1] <= tol * errs[0]:
                break
        return x, it, np.array(errs)
