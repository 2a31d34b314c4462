"""The dense inverse of the coarsest level formed on the device (dense_spd.hpp: blocked Gauss-Jordan in 64 x 64 tiles) at the
sizes test_large_coarsest_level_is_inverted_on_the_device (several tiles, padded) does not reach:

  nc      tiles   what it reaches
  40      1       one tile, padded: the three panel kernels are skipped, the padding rows carry a unit diagonal
  64      1       one tile, exact: the padding kernels touch nothing, the application is the unpadded GEMV
  128     2       two tiles, no padding
  2112    33      the stream synchronisation inside the sweep (every 32nd step)

and the refusal of a coarsest matrix that is not positive definite on its free dofs.  Two-level hierarchies by
reorder.hand_hierarchy around a piecewise-constant P with exactly nc columns (two fine rows per aggregate), so the coarsest size
is chosen; the hierarchy hands over no inverse (coarse_n == 0), amgx_create forms it.  The 40-unknown case also runs with a few
non-free coarse rows.  Bounds of the existing test: the cycle against the oracle at 1e-10, CoarseSolve with a residual of at most
1e-9 |r| on the free dofs and exact zeros elsewhere."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from ngsamg_amd._lib import Matrix, NgsAMGError
from tests import reorder as R

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _levels(nc):
    """level list of the two-level hierarchy with nc coarse unknowns (shared, read-only)"""
    n = 2 * nc
    A, _ = R.stencil("offsets:1,2,5", (n,), seed=nc)
    P = sp.csr_matrix((np.ones(n), (np.arange(n), np.arange(n) // 2)), shape=(n, nc))
    return R.hand_hierarchy(A, per_row=(), first_P=[P]).levels


def _hierarchy(nc, nonfree=(), coarse_A=None):
    """a hierarchy over (shallow copies of) the shared levels that hands over no coarse inverse"""
    import copy
    from tests.test_gpu_kernel_zoo import _H
    levels = [copy.copy(lv) for lv in _levels(nc)]
    if len(nonfree):
        levels[-1].free = levels[-1].free.copy()
        levels[-1].free[list(nonfree)] = 0
    if coarse_A is not None:
        levels[-1].A = coarse_A
    H = _H(levels)
    assert H.n_levels == 2 and H.coarse_n == 0 and levels[-1].A.n_rows == nc and levels[-1].A.br == 1
    return H


@pytest.mark.parametrize("nc,nonfree", [(40, ()), (40, (0, 7, 39)), (64, ()), (128, ()), (2112, ())])
def test_coarsest_level_inverse_sizes(nc, nonfree):
    from ngsamg_amd.device import DeviceAMGMatrix
    from oracle.pyoracle import Oracle
    H = _hierarchy(nc, nonfree)
    dev = DeviceAMGMatrix(H, sm_type="jacobi", clev="inv", device=0)
    assert dev.sizes[-1] == nc and dev.cycle_info()["dense_level"] == -1
    rng = np.random.default_rng(nc)
    n = dev.sizes[0]
    b = rng.standard_normal(n)
    x = np.empty(n)
    dev.Mult(b, x)
    ref = Oracle(H.levels, sm_type="jacobi").apply(b)
    ec = np.linalg.norm(x - ref) / np.linalg.norm(ref)
    f = H.levels[-1].free.astype(bool)
    r = rng.standard_normal(nc) * f
    xc = np.empty(nc)
    dev.CoarseSolve(r, xc)
    Ac = H.levels[-1].A.to_scipy()
    er = np.linalg.norm((Ac @ xc - r)[f]) / np.linalg.norm(r)
    print(f"nc={nc} non-free={len(nonfree)}: cycle {ec:.2e}, coarse solve residual {er:.2e}")
    assert ec <= 1e-10
    assert er <= 1e-9 and np.all(xc[~f] == 0.0)


@pytest.mark.parametrize("nc,row", [(40, 5), (128, 100)])
def test_indefinite_coarsest_matrix_is_refused(nc, row):
    """one diagonal entry with the wrong sign (in the first tile / in the second, after a trailing update): a negative pivot,
    amgx_create returns the error"""
    from ngsamg_amd.device import DeviceAMGMatrix
    Ac = _levels(nc)[-1].A.to_scipy().tolil()
    Ac[row, row] = -Ac[row, row]
    H = _hierarchy(nc, coarse_A=Matrix.from_scipy(Ac.tocsr()))
    with pytest.raises(NgsAMGError, match="not positive definite"):
        DeviceAMGMatrix(H, sm_type="jacobi", clev="inv", device=0)
