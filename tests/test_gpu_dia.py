"""The symmetric diagonal (DIA) image of level 0 for the fused Jacobi down pass (dia_pre_restrict_kernel): cycles against
the oracle and against the SELL path of the same hierarchy (AMGX_NO_DIA=1), PCG iteration counts, device vs host image.
The size threshold (AMGX_DIA_MIN_ROWS, 2 M rows by default) is lowered so that small Kuhn problems take the path."""
import numpy as np
import pytest

from tests.problems import poisson_case, rhs

pytestmark = pytest.mark.gpu

# (shape, Dirichlet, max_coarse_size): grids that are not multiples of 64 / 512 in any direction, 3D and 2D
CASES = [((41, 37, 29), "right|top", 10), ((130, 110), "left|top", 5)]


def _rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def _dev(H, monkeypatch, env=(), **kw):
    from ngsamg_amd.device import DeviceAMGMatrix
    with monkeypatch.context() as m:
        m.setenv("AMGX_DIA_MIN_ROWS", "0")
        for k, v in env:
            m.setenv(k, v)
        return DeviceAMGMatrix(H, device=0, sm_type="jacobi", **kw)


def _apply(dev, b):
    x = np.full(b.size, np.nan)
    dev.Mult(b, x)
    return x


@pytest.mark.parametrize("shape,diri,mcs", CASES)
@pytest.mark.parametrize("cycle", ["V", "W", "BS"])
def test_dia_cycles_match_oracle_and_sell_path(shape, diri, mcs, cycle, monkeypatch):
    from oracle.pyoracle import Oracle
    p, H = poisson_case(shape, diri, mcs)
    b = rhs(p, 1)
    ref = Oracle(H.levels, sm_type="jacobi", cycle=cycle).apply(b)
    dev = _dev(H, monkeypatch, mg_cycle=cycle)
    assert dev.matrix_info(0, "Apre")["fmt"] == "dia"
    assert dev.matrix_info(0, "Apre")["stored"] == (7 if len(shape) == 3 else 3) * p.n
    x = _apply(dev, b)
    assert _rel(x, ref) < 1e-12
    sell = _dev(H, monkeypatch, env=[("AMGX_NO_DIA", "1")], mg_cycle=cycle)
    assert sell.matrix_info(0, "Apre")["fmt"] not in (None, "dia")
    assert _rel(x, _apply(sell, b)) < 1e-13
    # the literal (unfolded) V-cycle sequence on the same image
    if cycle == "V":
        nofold = _dev(H, monkeypatch, env=[("AMGX_NO_FOLD", "1")])
        assert nofold.matrix_info(0, "Apre")["fmt"] == "dia"
        assert _rel(_apply(nofold, b), ref) < 1e-12
        # compact chunks (on by default from 200 k rows) on the same image
        compact = _dev(H, monkeypatch, env=[("AMGX_COMPACT_CHUNKS_MIN_ROWS", "0")])
        assert compact.level_paths(0)["kernel"] == "dia" and compact.level_paths(0)["compact"] == 1
        assert dev.level_paths(0)["compact"] == 0
        assert _rel(_apply(compact, b), x) < 1e-13
    # levels >= 1 (aggregated, not on <= 16 diagonals) keep their formats
    for l in range(1, dev.GetNLevels() - 1):
        assert dev.matrix_info(l, "Apre") == sell.matrix_info(l, "Apre")


@pytest.mark.parametrize("shape,diri,mcs", CASES)
def test_dia_device_image_equals_host_image(shape, diri, mcs, monkeypatch):
    """AMGX_VERIFY_IMAGES compares the device-built image with the host builder bit for bit (and raises if they differ);
    host-built images (AMGX_HOST_IMAGES) give the same image, hence the same result bit for bit"""
    p, H = poisson_case(shape, diri, mcs)
    b = rhs(p, 2)
    small = [("AMGX_DEV_IMAGES_MIN_ROWS", "0")]
    xv = _apply(_dev(H, monkeypatch, env=small + [("AMGX_VERIFY_IMAGES", "1")]), b)
    dh = _dev(H, monkeypatch, env=[("AMGX_HOST_IMAGES", "1")])
    assert dh.matrix_info(0, "Apre")["fmt"] == "dia"
    xd = _apply(_dev(H, monkeypatch, env=small), b)
    assert np.array_equal(xv, _apply(dh, b)) and np.array_equal(xv, xd)


def test_dia_pcg_iterations_equal_oracle(monkeypatch):
    import torch
    from oracle.pyoracle import Oracle
    from ngsamg_amd.krylov import CGSolver
    p, H = poisson_case((41, 37, 29), "right|top", 10)
    _, it_ref, _ = Oracle(H.levels, sm_type="jacobi").pcg(p.load, tol=1e-10, maxit=200)
    dev = _dev(H, monkeypatch)
    assert dev.matrix_info(0, "Apre")["fmt"] == "dia"
    cg = CGSolver(dev, dev, tol=1e-10, maxsteps=200)
    cg.Solve(torch.from_numpy(p.load).cuda())
    assert cg.iterations == it_ref


def test_dia_fused_kernel_timed_and_size_threshold(monkeypatch):
    """amgx_time_op ops 5 / 7 run the diagonal-image kernel; below the size threshold level 0 keeps its old format"""
    p, H = poisson_case((41, 37, 29), "right|top", 10)
    dev = _dev(H, monkeypatch)
    assert dev.time_op(0, 7, reps=2) > 0 and dev.time_op(0, 5, reps=2) > 0
    # default threshold: a 44 k-row level keeps its image of A'
    from ngsamg_amd.device import DeviceAMGMatrix
    assert DeviceAMGMatrix(H, device=0, sm_type="jacobi").matrix_info(0, "Apre")["fmt"] not in (None, "dia")
