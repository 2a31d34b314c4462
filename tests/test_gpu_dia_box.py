"""Box chunks of the level-0 diagonal image (dia_box_pre_restrict_kernel): a workgroup owns a box of whole grid lines and takes
the in-box neighbours' x from LDS.  Cycles against the oracle, and the down pass against the 512-row chunks of the same hierarchy
(AMGX_NO_DIA_BOX=1): the stored x bit for bit, b_coarse up to the regrouped partial sums.  Both size thresholds are lowered to 0,
and the fill threshold of the image is raised (AMGX_DIA_MAX_FILL): the three thin grids store 1.09 to 1.24 entries per entry of A,
above the default 1.05, and would keep the SELL image.

Grids (nx, ny, nz), x fastest: (70, 5, 6) -- two waves per line, the second partial; ny odd, so the last box in y is a single line,
and the second box in z holds two planes --, (9, 9, 9), (130, 7) -- 2D, one clipped box --, and the two cases of
tests/test_gpu_dia.py.  fem.poisson_fast numbers the LAST direction of its shape fastest, so the shapes below are the grids reversed.

The literal sequence (AMGX_NO_FOLD=1) has no stage entry point for the fused down pass (amgx_cycle_down needs the folded
level), so there the whole V-cycle of the two handles is compared: it differs by the regrouped partial sums alone, which are
rounding differences of sums of ~10 terms (1e-13 relative)."""
import functools

import numpy as np
import pytest

from tests import reorder as R
from tests.problems import poisson_case, rhs

pytestmark = pytest.mark.gpu

# (shape, Dirichlet, max_coarse_size)
CASES = [((6, 5, 70), "right|top", 10), ((9, 9, 9), "right|top", 10), ((7, 130), "left|top", 5), ((41, 37, 29), "right|top", 10),
         ((130, 110), "left|top", 5)]
BOX = (("AMGX_DIA_MIN_ROWS", "0"), ("AMGX_DIA_BOX_MIN_ROWS", "0"), ("AMGX_DIA_MAX_FILL", "1.5"))
OLD = BOX + (("AMGX_NO_DIA_BOX", "1"),)


def _rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def _dev(H, monkeypatch, env, **kw):
    from ngsamg_amd.device import DeviceAMGMatrix
    with monkeypatch.context() as m:
        for k, v in env:
            m.setenv(k, v)
        return DeviceAMGMatrix(H, device=0, sm_type="jacobi", **kw)


def _apply(dev, b):
    x = np.full(b.size, np.nan)
    dev.Mult(b, x)
    return x


def _down(dev, b):
    z, bc = np.full(dev.sizes[0], np.nan), np.full(dev.sizes[1], np.nan)
    dev.CycleDown(0, b, z, bc)
    return z, bc


@functools.lru_cache(maxsize=None)
def _oracle(shape, diri, mcs, cycle):
    from oracle.pyoracle import Oracle
    p, H = poisson_case(shape, diri, mcs)
    ref = Oracle(H.levels, sm_type="jacobi", cycle=cycle).apply(rhs(p, 1))
    ref.setflags(write=False)
    return ref


def _check_down(box, old, b):
    z, bc = _down(box, b)
    z0, bc0 = _down(old, b)
    assert np.array_equal(z, z0)
    assert _rel(bc, bc0) < 1e-13


@pytest.mark.parametrize("shape,diri,mcs", CASES)
def test_box_cycle_matches_oracle_and_down_pass_matches_row_chunks(shape, diri, mcs, monkeypatch):
    p, H = poisson_case(shape, diri, mcs)
    b = rhs(p, 1)
    box = _dev(H, monkeypatch, BOX)
    lp = box.level_paths(0)
    assert lp["kernel"] == "dia" and lp["compact"] == 2, lp
    assert lp["fused_block"] == 512 and lp["dia_k"] == (7 if len(shape) == 3 else 3)
    ny = shape[-2]
    nz = shape[0] if len(shape) == 3 else 1
    yc, zc = (2, 4) if len(shape) == 3 else (8, 1)
    assert lp["chunks"] == -(-ny // yc) * -(-nz // zc)
    assert _rel(_apply(box, b), _oracle(shape, diri, mcs, "V")) < 1e-12
    old = _dev(H, monkeypatch, OLD)
    assert old.level_paths(0)["kernel"] == "dia" and old.level_paths(0)["compact"] == 0
    _check_down(box, old, b)
    # no non-temporal epilogue operands, nothing hoisted
    env = (("AMGX_NO_EP_NT", "1"), ("AMGX_NO_EP_HOIST", "1"))
    _check_down(_dev(H, monkeypatch, BOX + env), _dev(H, monkeypatch, OLD + env), b)
    # the literal (unfolded) sequence: see the module docstring
    nf = _dev(H, monkeypatch, BOX + (("AMGX_NO_FOLD", "1"),))
    assert nf.level_paths(0)["compact"] == 2 and not nf.is_folded(0)
    x = _apply(nf, b)
    assert _rel(x, _oracle(shape, diri, mcs, "V")) < 1e-12
    assert _rel(x, _apply(_dev(H, monkeypatch, OLD + (("AMGX_NO_FOLD", "1"),)), b)) < 1e-13


@pytest.mark.parametrize("cycle", ["W", "BS"])
def test_box_w_and_bs_cycles_match_oracle(cycle, monkeypatch):
    shape, diri, mcs = CASES[0]
    p, H = poisson_case(shape, diri, mcs)
    dev = _dev(H, monkeypatch, BOX, mg_cycle=cycle)
    assert dev.level_paths(0)["compact"] == 2
    assert _rel(_apply(dev, rhs(p, 1)), _oracle(shape, diri, mcs, cycle)) < 1e-12


@pytest.mark.parametrize("yz", ["2x2", "1x4"])
def test_box_shape_hook(yz, monkeypatch):
    shape, diri, mcs = CASES[0]
    p, H = poisson_case(shape, diri, mcs)
    b = rhs(p, 1)
    dev = _dev(H, monkeypatch, BOX + (("AMGX_DIA_BOX_SHAPE", yz),))
    yc, zc = (int(v) for v in yz.split("x"))
    lp = dev.level_paths(0)
    assert lp["compact"] == 2 and lp["chunks"] == -(-shape[1] // yc) * -(-shape[0] // zc), lp
    _check_down(dev, _dev(H, monkeypatch, OLD), b)


def test_box_prolongation_with_five_entries_per_row(monkeypatch):
    """the dia-ept6 construction of tests/test_gpu_down_family.py: 7-point stencil, 5 entries of P per row -- 1640 entries in a box
    of 328 rows"""
    from oracle.pyoracle import Oracle
    from tests.test_gpu_down_family import _fd7
    H, b = _fd7((5, 2))
    box = _dev(H, monkeypatch, BOX)
    lp = box.level_paths(0)
    assert lp["kernel"] == "dia" and lp["compact"] == 2 and lp["dia_k"] == 3 and lp["max_entries"] > 3 * 41 * 8, lp
    assert _rel(_apply(box, b), Oracle(H.levels, sm_type="jacobi").apply(b)) < 1e-12
    _check_down(box, _dev(H, monkeypatch, OLD), b)


def test_box_refused_matrix_keeps_row_chunks_bit_for_bit(monkeypatch):
    """the 9-point stencil of tests/reorder.py has the offset nx - 1: a diagonal image, but no grid the boxes know"""
    A, _ = R.stencil("fd9", (130, 110), seed=4)
    H = R.hand_hierarchy(A, per_row=(2, 2), agg=8, seed=4)
    b = np.random.default_rng(4).standard_normal(A.shape[0])
    dev, old = _dev(H, monkeypatch, BOX), _dev(H, monkeypatch, OLD)
    assert dev.level_paths(0)["kernel"] == "dia" and dev.level_paths(0)["compact"] != 2
    assert dev.level_paths(0) == old.level_paths(0)
    assert np.array_equal(_apply(dev, b), _apply(old, b))
    z, bc = _down(dev, b)
    z0, bc0 = _down(old, b)
    assert np.array_equal(z, z0) and np.array_equal(bc, bc0)


def test_box_kernel_timed_and_size_threshold(monkeypatch):
    shape, diri, mcs = CASES[0]
    p, H = poisson_case(shape, diri, mcs)
    dev = _dev(H, monkeypatch, BOX)
    assert dev.time_op(0, 7, reps=2) > 0 and dev.time_op(0, 8, reps=2) > 0
    # default threshold (200 k rows): a small level keeps the chunks it has today
    small = _dev(H, monkeypatch, (("AMGX_DIA_MIN_ROWS", "0"), ("AMGX_DIA_MAX_FILL", "1.5")))
    assert small.level_paths(0)["kernel"] == "dia" and small.level_paths(0)["compact"] == 0
