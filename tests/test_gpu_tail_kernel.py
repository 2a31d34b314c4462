"""The single-workgroup coarse tail (tail_kernel, kernels.hpp) on hierarchies whose level sizes are chosen.

By default the collapsed dense operator replaces the tail, so every handle here is built with AMGX_NO_DENSE_TAIL=1, a V-cycle and
clev = "inv", and every case first asserts cycle_info(): tail_level == 1, dense_level == -1.  Scalar hierarchies by
reorder.hand_hierarchy around piecewise-constant prolongations (consecutive rows share an aggregate) with a valid colouring of every
level; the hierarchy hands over the coarse inverse (the tail needs an unpadded one).  What the cases reach:

  T_GS, x in LDS            a tail level of <= 128 rows of <= 64 entries (level_extra: tail_gs_lds == 1)
  T_GS, x in global memory  AMGX_NO_TAIL_LDS=1 on the same level; a level of 250 rows; a level with rows of more than 64 entries
  T_SPMV, rolled remainder  rows of 65, 72 and 100 entries (more than TAIL_SP_K * TAIL_G = 64)
  ops[i] from global memory a program of 49 operations (TAIL_MAX_OPS = 48 are staged in LDS), and its neighbour of 47
  rows that are not swept   colour -1 on a tail level
  AMGX_NO_TAIL_KERNEL=1     the same levels as separate launches

Bounds: the oracle at 1e-12 (Jacobi) / 1e-10 (Gauss-Seidel, gs_mc), separate launches against the tail at the 1e-13 mutual bound
between launch forms (test_gpu_dense_tail.py).  A second application of every handle must repeat the first bit for bit."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import scipy.sparse as sp

from tests import reorder as R
from tests.problems import rhs
from tests.test_gpu_devbuild import env

pytestmark = pytest.mark.gpu

TOL = {"jacobi": 1e-12, "gs": 1e-10}
OSM = {"jacobi": "jacobi", "gs": "gs_mc"}


def _rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def _agg(n, nc):
    """n x nc, piecewise constant: row i belongs to aggregate i * nc // n (consecutive rows together)"""
    return sp.csr_matrix((np.ones(n), (np.arange(n), np.arange(n) * nc // n)), shape=(n, nc))


def _hierarchy(sizes, A=None, nonfree=None):
    """levels of sizes[0], sizes[1], ... rows around A (default: couplings i -- i + 1, 2, 5); nonfree = (level, rows): those rows
    of that level are not free, get colour -1, a zero inverse diagonal and an empty row in the prolongation from the next level,
    so that x stays 0 on them as on the non-free rows of a hierarchy of the host setup (the split Gauss-Seidel images drop the
    couplings to such columns: gs_images.hpp, colour_part)"""
    if A is None:
        A, _ = R.stencil("offsets:1,2,5", (sizes[0],), seed=sizes[0])
    Ps = [_agg(a, b) for a, b in zip(sizes[:-1], sizes[1:])]
    if nonfree is not None:
        l, rows = nonfree
        assert 0 < l < len(sizes) - 1
        keep = np.ones(sizes[l])
        keep[list(rows)] = 0.0
        Ps[l] = (sp.diags(keep) @ Ps[l]).tocsr()
        Ps[l].eliminate_zeros()
        assert np.all(np.diff(Ps[l].tocsc().indptr) > 0)        # no aggregate lost all its rows
    H = R.hand_hierarchy(A, per_row=(), first_P=Ps)
    assert [lv.n for lv in H.levels] == list(sizes)
    for l, lv in enumerate(H.levels):
        if nonfree is not None and nonfree[0] == l:
            lv.free[list(nonfree[1])] = 0
            lv.dinv[list(nonfree[1])] = 0.0
        lv.color, lv.n_colors = R.coloring(lv.A, lv.free)
    return H


@functools.lru_cache(maxsize=None)
def _case(name):
    """(hierarchy, right-hand side); shared and read-only"""
    if name == "lds":                   # level 1: 100 <= 128 rows of <= 64 entries
        H = _hierarchy((200, 100, 40))
    elif name == "global":              # level 1: 250 > 128 rows
        H = _hierarchy((500, 250, 40))
    elif name == "nonfree":
        H = _hierarchy((200, 100, 40), nonfree=(1, (0, 17, 18, 63, 99)))
    elif name == "long_rows":
        H = _hierarchy((240, 120, 30), A=_long_row_fine_matrix())
    elif name == "ops49":
        H = _hierarchy((512, 256, 128, 64, 32, 16, 8, 4, 2, 1))
    else:
        raise ValueError(name)
    p = SimpleNamespace(n=H.levels[0].n, bs=1, free=H.levels[0].free)
    return H, rhs(p, 7)


LONG = {10: 65, 50: 72, 90: 100}        # coarse row -> entries


def _long_row_fine_matrix():
    """240 fine rows, couplings i -- i + 1, 2 (coarse rows of 3 entries under the pairwise aggregation) and, for the coarse rows r
    of LONG, couplings of fine row 2 r to one fine row of as many further aggregates as the row needs; the long rows do not couple
    to each other"""
    n = 240
    rng = np.random.default_rng(5)
    I = [np.arange(n - 1), np.arange(n - 2)]
    J = [np.arange(1, n), np.arange(2, n)]
    for r, want in LONG.items():
        others = [a for a in range(n // 2) if abs(a - r) > 1 and a not in LONG][:want - 3]
        I.append(np.full(len(others), 2 * r))
        J.append(2 * np.asarray(others) + 1)
    I, J = np.concatenate(I), np.concatenate(J)
    lo, hi = np.minimum(I, J), np.maximum(I, J)
    return R._assemble(n, lo, hi, rng.uniform(0.5, 1.5, size=I.size), 0.05)


def _dev(H, sm, **e):
    from ngsamg_amd.device import DeviceAMGMatrix
    with env(AMGX_NO_DENSE_TAIL=1, **e):
        return DeviceAMGMatrix(H, sm_type=sm, mg_cycle="V", clev="inv", device=0)


def _tail(H, sm, **e):
    """a handle whose levels >= 1 run inside tail_kernel (asserted), and the lds flags of its tail levels"""
    d = _dev(H, sm, **e)
    ci = d.cycle_info()
    assert ci["tail_level"] == 1 and ci["dense_level"] == -1, ci
    lds = [d.level_extra(l)["tail_gs_lds"] for l in range(1, H.n_levels - 1)]
    assert d.level_extra(0)["tail_gs_lds"] is None and d.level_extra(H.n_levels - 1)["tail_gs_lds"] is None
    return d, lds


def _apply_twice(d, b):
    x1, x2 = np.full(b.size, np.nan), np.full(b.size, np.nan)
    d.Mult(b, x1)
    d.Mult(b, x2)
    assert np.array_equal(x1, x2)           # the work vectors of the tail are clean again
    return x1


def _oracle(H, types, b):
    from oracle.pyoracle import Oracle
    return Oracle(H.levels, sm_type=[OSM[t] for t in types] if isinstance(types, list) else OSM[types]).apply(b)


@pytest.mark.parametrize("name", ["lds", "global", "nonfree"])
@pytest.mark.parametrize("sm", ["jacobi", "gs"])
def test_tail_forms_match_oracle_and_each_other(name, sm):
    """Both T_GS forms add a row's entries alike -- lane `sub` of the row's 8 lanes takes the entries sub, sub + 8, ... in this order
    from 0.0 (the LDS form's padding adds 0 * x, which changes no bit of a finite sum), then the same xor tree over 8 lanes -- and
    update x[row] += dinv * (b - acc) from the same operands, so AMGX_NO_TAIL_LDS=1 must reproduce the LDS form bit for bit.
    Rows of colour -1 are in no colour's list (global form) and match no colour (LDS form): they keep x (0 in a cycle, as the
    prolongation has empty rows there).  Separate launches
    (AMGX_NO_TAIL_KERNEL=1) use other kernels with other summation orders: the 1e-13 bound between launch forms."""
    H, b = _case(name)
    d, lds = _tail(H, sm)
    want = [None] if sm == "jacobi" else [0 if name == "global" else 1]
    assert lds == want, lds
    assert d.level_extra(1)["tail_ops"] == (5 if sm == "jacobi" else 7)
    x = _apply_twice(d, b)
    ref = _oracle(H, sm, b)
    e_ref = _rel(x, ref)
    dg, ldsg = _tail(H, sm, AMGX_NO_TAIL_LDS=1)
    assert ldsg == ([None] if sm == "jacobi" else [0])
    xg = _apply_twice(dg, b)
    ds = _dev(H, sm, AMGX_NO_TAIL_KERNEL=1)
    cs = ds.cycle_info()
    assert cs["tail_level"] == -1 and cs["dense_level"] == -1 and ds.level_extra(1)["tail_ops"] == 0
    xs = _apply_twice(ds, b)
    e_sep = _rel(xs, x)
    print(f"{name} {sm}: tail vs oracle {e_ref:.2e}, separate launches vs tail {e_sep:.2e}, separate vs oracle {_rel(xs, ref):.2e}")
    assert e_ref <= TOL[sm] and _rel(xs, ref) <= TOL[sm]
    assert np.array_equal(xg, x)
    assert e_sep <= 1e-13
    if name == "nonfree":
        assert H.levels[1].n_colors >= 2 and np.count_nonzero(H.levels[1].color < 0) == 5


@pytest.mark.parametrize("sm", ["jacobi", "gs"])
def test_tail_rows_beyond_64_entries(sm):
    """rows of 65, 72 and 100 entries on the tail level: the T_SPMV branch keeps 8 entries per lane in registers and takes the rest in
    its rolled loop (remainders of 1, 8 and 36 entries: one lane, all lanes once, up to five trips), and a Gauss-Seidel sweep cannot
    keep such a row in registers, so it takes the global form without any switch"""
    H, b = _case("long_rows")
    lens = np.diff(H.levels[1].A.rowptr)
    assert sorted(int(v) for v in lens[lens > 8]) == sorted(LONG.values()) and all(int(lens[r]) == w for r, w in LONG.items())
    assert lens.size == 120 and np.count_nonzero(lens < 8) == 117
    d, lds = _tail(H, sm)
    assert lds == ([None] if sm == "jacobi" else [0])
    x = _apply_twice(d, b)
    ref = _oracle(H, sm, b)
    xs = _apply_twice(_dev(H, sm, AMGX_NO_TAIL_KERNEL=1), b)
    print(f"long rows {sm}: tail vs oracle {_rel(x, ref):.2e}, separate launches vs tail {_rel(xs, x):.2e}")
    assert _rel(x, ref) <= TOL[sm]
    assert _rel(xs, x) <= 1e-13


@pytest.mark.parametrize("types,ops", [(["gs"] * 10, 49), (["gs"] * 4 + ["jacobi"] + ["gs"] * 5, 47)])
def test_tail_program_longer_than_the_staged_operations(types, ops):
    """eight smoothed tail levels of 256 .. 2 rows and a coarsest level of one row.  A Gauss-Seidel level costs 4 operations going
    down (zero, sweep, residual, restriction) and 2 going up (prolongation, sweep), a Jacobi level 2 + 2, the coarse solve 1:
    8 x 6 + 1 = 49 operations, one more than TAIL_MAX_OPS = 48, so the last one (the backward sweep of level 1) is read from global
    memory; with one Jacobi level the program has 47 and is staged whole."""
    H, b = _case("ops49")
    d, lds = _tail(H, types)
    assert d.level_extra(0)["tail_ops"] == ops
    assert lds == [None if t == "jacobi" else (0 if H.levels[l + 1].n > 128 else 1) for l, t in enumerate(types[1:-1])]
    x = _apply_twice(d, b)
    ref = _oracle(H, types, b)
    xs = _apply_twice(_dev(H, types, AMGX_NO_TAIL_KERNEL=1), b)
    print(f"{ops} operations: tail vs oracle {_rel(x, ref):.2e}, separate launches vs tail {_rel(xs, x):.2e}")
    assert _rel(x, ref) <= 1e-10
    assert _rel(xs, x) <= 1e-13
