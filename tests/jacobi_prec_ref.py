"""The definition of single-precision Jacobi images (jacobi_prec = "single"), for the tests: a numpy emulation of the
folded scalar Jacobi V-cycle whose matrix images are rounded AS STORED.  Per smoothed level, with D^-1 = diag(dinv):

    down   x_pre = omega D^-1 b;   r = b - A' b;   z = x_pre + omega D^-1 r;   b_c = P^T r
    up     x = z + Q x_c

    A' = A diag(omega dinv)      formed in fp64, every entry through float32 -- the diagonal a_ii omega dinv_i = omega included, whose
                                 rounding (float32(0.9) - 0.9 = -2.4e-8) is the same on every row
    Q  = P - omega D^-1 A P      formed in fp64, every entry through float32

form = "apre_wd": A' in the one-thread-per-row form whose diagonal slot carries omega dinv_i (wdiag: AMGX levels built on the device and
one-lane host-built ones): the kernel puts the diagonal term back as omega b_i in fp64, the slot goes through float32 with the image,
and the kernels take the Dinv of the own row from it, dinv_i = float32(omega dinv_i) / omega, in x_pre and z -- the one place where the
device's Dinv is not the fp64 array.
form = "dia": the level streams the symmetric diagonal image instead of A' -- the entries of A itself go through float32 and the
neighbours' x_j = omega (dinv_j b_j) are formed in fp64.  Vectors, dinv, P^T, the coarse inverse and every sum stay fp64.
form = "double": nothing of the level is rounded (the levels inside the single-workgroup tail program keep fp64 copies).
round32=False gives the same cycle in fp64: the double handle's arithmetic up to the order of additions.

The literal cycle (AMGX_NO_FOLD=1 and no A') is the fp64 cycle on tests/mat_prec_ref.RoundedHierarchy.

    FoldedJacobiRef(H, omega, round32, forms).apply(b)
    symmetry_defect(cycle, n, seed)      |<Cx, y> - <x, Cy>| / (|Cx| |y|)
"""
import numpy as np
import scipy.sparse as sp


def _f32(v):
    return np.asarray(v, dtype=np.float64).astype(np.float32).astype(np.float64)


class FoldedJacobiRef:
    def __init__(self, H, omega=0.9, round32=True, forms=None):
        self.L = len(H.levels)
        self.omega = float(omega)
        n = int(H.coarse_n)
        self.cinv = np.asarray(H.coarse_inv, dtype=np.float64).reshape(n, n)
        forms = list(forms) if forms is not None else ["apre"] * (self.L - 1)
        self.lv = []
        for l in range(self.L - 1):
            lv = H.levels[l]
            A = lv.A.to_scipy().tocsr()
            P = lv.P.to_scipy().tocsr()
            dinv = np.asarray(lv.dinv, dtype=np.float64)
            r32 = round32 and forms[l] != "double"
            w = self.omega * dinv
            Q = (P - sp.diags(w) @ (A @ P)).tocsr()
            if forms[l] == "dia":
                N = (A - sp.diags(A.diagonal())).tocsr()          # the couplings; x_j = omega (dinv_j b_j) is formed per entry
                if r32:
                    N.data = _f32(N.data)
                off = (N @ sp.diags(w)).tocsr()
            else:
                off = (A @ sp.diags(w)).tocsr()
                if forms[l] == "apre_wd":
                    off = (off - sp.diags(off.diagonal())).tocsr()
                if r32:
                    off.data = _f32(off.data)
            if r32:
                Q.data = _f32(Q.data)
            own = _f32(w) / self.omega if (forms[l] == "apre_wd" and r32) else dinv       # Dinv of the own row in the Jacobi store
            self.lv.append(dict(off=off, Q=Q, PT=lv.PT.to_scipy().tocsr(), dinv=own, diag=(dinv != 0.0).astype(np.float64) if forms[l] in ("apre_wd", "dia") else np.zeros_like(dinv)))

    def _cycle(self, l, b):
        if l == self.L - 1:
            return self.cinv @ b
        v, om = self.lv[l], self.omega
        x_pre = om * (v["dinv"] * b)
        r = b - (v["off"] @ b + om * (v["diag"] * b))
        z = x_pre + om * (v["dinv"] * r)
        xc = self._cycle(l + 1, v["PT"] @ r)
        return z + v["Q"] @ xc

    def apply(self, b):
        return self._cycle(0, np.asarray(b, dtype=np.float64))


def symmetry_defect(cycle, n, seed=7):
    rng = np.random.default_rng(seed)
    x, y = rng.standard_normal(n), rng.standard_normal(n)
    cx, cy = cycle.apply(x), cycle.apply(y)
    return abs(float(cx @ y) - float(x @ cy)) / (np.linalg.norm(cx) * np.linalg.norm(y))
