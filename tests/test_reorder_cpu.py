"""The reordering helpers of tests/reorder.py, checked on the CPU: the oracle on a renumbered hierarchy is the renumbered oracle
result (only summation orders differ), so the GPU tests of tests/test_gpu_reorder.py can take it as their reference."""
import numpy as np
import pytest

from tests import reorder as R
from tests.problems import elasticity_case, poisson_case, rhs

CASES = {"p3": lambda: poisson_case((41, 37, 29), "right|top", 10), "p2": lambda: poisson_case((130, 110), "left|top", 5),
         "e3": lambda: elasticity_case((9, 8, 7)), "e6": lambda: elasticity_case((9, 8, 7), rotations=True)}


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("name", list(CASES))
def test_oracle_is_equivariant(name, kind):
    from oracle.pyoracle import Oracle
    p, H = CASES[name]()
    perms = R.level_perms(H, kind, seed=7)
    Hp = R.permute_hierarchy(H, perms)
    b = rhs(p, 1)
    bp = R.permute_vec(b, perms[0], p.bs)
    for cycle in ("V", "W", "BS"):
        ref = R.permute_vec(Oracle(H.levels, sm_type="jacobi", cycle=cycle).apply(b), perms[0], p.bs)
        x = Oracle(Hp.levels, sm_type="jacobi", cycle=cycle).apply(bp)
        assert np.linalg.norm(x - ref) <= 1e-13 * np.linalg.norm(ref), cycle


@pytest.mark.parametrize("kind", ["random", "rcm", "coarse_only"])
def test_permuted_levels_are_the_permuted_operators(kind):
    """A' = Pi A Pi^T, P' = Pi_0 P Pi_1^T, P'^T = (P')^T exactly, with sorted columns; block levels move whole blocks"""
    for name in ("p2", "e6"):
        p, H = CASES[name]()
        perms = R.level_perms(H, kind, seed=3)
        Hp = R.permute_hierarchy(H, perms)
        for l, (a, c) in enumerate(zip(H.levels, Hp.levels)):
            bs = a.A.br
            ex = lambda q: np.repeat(np.asarray(q) * bs, bs) + np.tile(np.arange(bs), len(q))
            p0 = ex(perms[l])
            assert (c.A.to_scipy() != a.A.to_scipy()[p0][:, p0]).nnz == 0
            for i in range(c.A.n_rows):
                seg = c.A.col[c.A.rowptr[i]:c.A.rowptr[i + 1]]
                assert np.all(np.diff(seg) > 0)
            if a.P is not None:
                p1 = np.repeat(np.asarray(perms[l + 1]) * a.P.bc, a.P.bc) + np.tile(np.arange(a.P.bc), len(perms[l + 1]))
                assert (c.P.to_scipy() != a.P.to_scipy()[p0][:, p1]).nnz == 0
                assert (c.PT.to_scipy() != c.P.to_scipy().T).nnz == 0
            assert np.array_equal(c.free, np.asarray(a.free)[perms[l]])
            assert np.array_equal(c.dinv, np.asarray(a.dinv).reshape(a.A.n_rows, -1)[perms[l]].reshape(-1))


def test_permutation_kinds():
    n = 1500
    for kind in R.KINDS:
        p = R.permutation(kind, n, seed=1, A=R.stencil("chain", (n,))[0])
        assert np.array_equal(np.sort(p), np.arange(n)), kind
    p = R.permutation("slice64", n, seed=1)
    assert np.array_equal(p // 64, np.arange(n) // 64) and not np.array_equal(p, np.arange(n))
    p = R.permutation("chunk512", n, seed=1)
    assert np.array_equal(p // 512, np.arange(n) // 512) and not np.array_equal(p, np.arange(n))


def test_hand_hierarchy_levels():
    A, _ = R.stencil("fd5", (60, 50))
    H = R.hand_hierarchy(A, per_row=(5, 2), agg=8)
    assert H.n_levels == 3
    assert np.all(np.diff(H.levels[0].P.rowptr) == 5) and np.all(np.diff(H.levels[1].P.rowptr) == 2)
    for l in range(2):
        Ac = (H.levels[l].PT.to_scipy() @ H.levels[l].A.to_scipy() @ H.levels[l].P.to_scipy())
        assert abs(Ac - H.levels[l + 1].A.to_scipy()).max() < 1e-13 * abs(Ac).max()
        assert np.array_equal(H.levels[l].dinv, 1.0 / H.levels[l].A.to_scipy().diagonal())
