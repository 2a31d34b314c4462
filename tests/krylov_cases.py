"""Shared pieces of the Krylov solver tests (tests/test_krylov_cpu.py, tests/test_gpu_krylov_edges.py, tests/test_gpu_dist.py):
a second, independent statement of the PCG recurrence in plain numpy, the initial guesses, the integer right-hand sides whose
inner products are exact in any summation order, and thin wrappers around the native solvers."""
import math
import os

import numpy as np

from tests.problems import elasticity_case, poisson_case

# vertex counts at the edges of the three regimes of the reductions (BLOCK = 256 lanes, KR_BLOCKS = 1024 workgroups):
# one workgroup (n <= 256, with n % 64 != 0 tails), one element per thread (n <= 262 144), grid-stride with a capped grid
EDGE_SHAPES = [(3, 3), (7, 9), (8, 8), (5, 13), (15, 17), (16, 16), (2, 129), (64, 64, 64), (65, 65, 63)]
EDGE_N = {(3, 3): 9, (7, 9): 63, (8, 8): 64, (5, 13): 65, (15, 17): 255, (16, 16): 256, (2, 129): 258, (64, 64, 64): 262144,
          (65, 65, 63): 266175}
SPIKE_ROWS = (0, 63, 64, 255, 256)        # plus n - 1


def edge_case(shape):
    p, H = poisson_case(shape, "right|top", 20)
    assert p.n == EDGE_N[shape]
    return p, H


def elasticity3():
    return elasticity_case((9, 9, 9), rotations=False, max_coarse_size=5)       # 3x3 blocks, 2187 unknowns


def elasticity6():
    return elasticity_case((9, 9, 9), rotations=True, max_coarse_size=5)        # 6x6 blocks, 4374 unknowns


def free_mask(p):
    return np.repeat(np.asarray(p.free), p.bs).astype(np.float64)


def guess(p, seed=5):
    """x0 = 10 * standard_normal on the free dofs: err_0 then differs clearly from the cold start's (an unscaled guess changes it
    by 2 % on Poisson 25^3)"""
    return 10.0 * np.random.default_rng(seed).standard_normal(p.n * p.bs) * free_mask(p)


def numpy_pcg(A, C, b, x0, tol, maxit):
    """textbook preconditioned CG, err_k = sqrt(|<C r_k, r_k>|), stop at err_k <= tol err_0.  A: scipy matrix, C: callable."""
    x = np.array(x0, dtype=np.float64)
    d = b - A @ x
    w = C(d)
    s = w.copy()
    wd = w @ d
    errs = [math.sqrt(abs(wd))]
    it = 0
    if errs[0] > 0:
        for it in range(1, maxit + 1):
            q = A @ s
            alpha = wd / (s @ q)
            x += alpha * s
            d -= alpha * q
            w = C(d)
            wdn = w @ d
            s = w + (wdn / wd) * s
            wd = wdn
            errs.append(math.sqrt(abs(wd)))
            if errs[-1] <= tol * errs[0]:
                break
    return x, it, np.array(errs)


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(float(np.linalg.norm(b)), 1e-300))


# ---- integer right-hand sides: every product and every partial sum is an integer below 2^53, so <b, b> is exact whatever the
# order of the additions, and sqrt is correctly rounded on both sides ---------------------------------------------------------
def integer_vectors(n, seed=0):
    """(name, vector) pairs: all ones, unit spikes at the regime boundaries that exist, random integers in [-8, 8]"""
    out = [("ones", np.ones(n))]
    for r in sorted({r for r in SPIKE_ROWS + (n - 1,) if r < n}):
        v = np.zeros(n)
        v[r] = 3.0
        out.append((f"spike{r}", v))
    out.append(("randint", np.random.default_rng(seed).integers(-8, 9, size=n).astype(np.float64)))
    return out


def exact_norm(v):
    """sqrt of the integer sum of squares of an integer-valued vector"""
    s = sum(int(t) * int(t) for t in np.asarray(v).astype(np.int64).tolist())
    assert s < 2 ** 53
    return math.sqrt(float(s))


def fsum_norm2(v):
    """sum of squares of a float64 vector in extended precision (products in long double, math.fsum of their head and tail)"""
    q = np.asarray(v, dtype=np.longdouble) ** 2
    hi = q.astype(np.float64)
    lo = (q - hi.astype(np.longdouble)).astype(np.float64)
    return math.fsum(hi.tolist() + lo.tolist())


# ---- the native solvers -------------------------------------------------------------------------------------------------------
def device_handle(H, env=None, **kw):
    """DeviceAMGMatrix created with `env` in os.environ (restored afterwards: amgx_create reads the switches)"""
    from ngsamg_amd.device import DeviceAMGMatrix
    env = env or {}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return DeviceAMGMatrix(H, device=0, **kw)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def native_solve(dev, kind, b, x0=None, tol=1e-10, maxit=100, restart=30, pre=True, device_vectors=True):
    """kind: 'pcg' | 'pcg_sr' | 'gmres'.  Returns (x, iterations, errs) as numpy; x0 is not modified."""
    from ngsamg_amd.krylov import NativeCGSolver, NativeGMResSolver
    if kind == "gmres":
        sv = NativeGMResSolver(dev, dev if pre else None, tol=tol, maxsteps=maxit, restart=restart)
    else:
        sv = NativeCGSolver(dev, dev if pre else None, tol=tol, maxsteps=maxit, single_reduction=(kind == "pcg_sr"))
    b = np.ascontiguousarray(b, dtype=np.float64)
    x = np.zeros_like(b) if x0 is None else np.array(x0, dtype=np.float64)
    if device_vectors:
        import torch
        xd = torch.from_numpy(x).cuda()
        sv.Solve(torch.from_numpy(b).cuda(), xd)
        torch.cuda.synchronize()
        x = xd.cpu().numpy()
    else:
        sv.Solve(b, x)
    return x, sv.iterations, np.asarray(sv.errors)


def native_solve_multi(dev, B, X0=None, tol=1e-10, maxit=100, pre=True, interleaved=False, device_vectors=True):
    """amgx_pcg_multi on (k, n) data whatever the layout handed to the library.  Returns (X (k, n), iterations, [errs])."""
    from ngsamg_amd.krylov import NativeCGSolver
    sv = NativeCGSolver(dev, dev if pre else None, tol=tol, maxsteps=maxit)
    B = np.asarray(B, dtype=np.float64)
    X = np.zeros_like(B) if X0 is None else np.array(X0, dtype=np.float64)
    Bin = np.ascontiguousarray(B.T) if interleaved else np.ascontiguousarray(B)
    Xin = np.ascontiguousarray(X.T) if interleaved else np.ascontiguousarray(X)
    if device_vectors:
        import torch
        Xd = torch.from_numpy(Xin).cuda()
        sv.SolveMulti(torch.from_numpy(Bin).cuda(), Xd, interleaved=interleaved)
        torch.cuda.synchronize()
        Xin = Xd.cpu().numpy()
    else:
        sv.SolveMulti(Bin, Xin, interleaved=interleaved)
    X = np.ascontiguousarray(Xin.T) if interleaved else Xin
    return X, list(sv.iterations), [np.asarray(e) for e in sv.errors]
