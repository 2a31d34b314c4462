"""The builders of the Gauss-Seidel images (csrc/device/gs_images.hpp: build_gs, build_gsb, build_bgsb) through the C ABI, on
hand-made levels of 64 (block) rows whose descriptor fields the tests set themselves.

  refusals      an invalid colouring, block list or block colouring is refused by amgx_create with its message (host validation,
                before anything of the smoother data is launched), and a valid create in the same process succeeds afterwards
  branches      inputs on which a builder declines the split images, built by the device kernels (AMGX_DEV_IMAGES_MIN_ROWS=0, with
                AMGX_VERIFY_IMAGES=1: every device-built array against the host builder's) and by the host loops
                (AMGX_HOST_IMAGES=1): the same amgx_level_paths and the same cycle, bit for bit

profiles/r20/builder_branches.txt lists every branch of the three builders with the test that reaches it."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import reorder as R

pytestmark = pytest.mark.gpu

N = 64
B_SCALAR = 16                  # rows per block of the scalar hybrid form: 16 lanes per row make the 256-lane workgroup
BS, BB = 3, 21                 # block size, block rows per sweep block (one BSELL slice of 64 // 3 block rows)
DEVICE = (("AMGX_DEV_IMAGES_MIN_ROWS", "0"), ("AMGX_VERIFY_IMAGES", "1"))
HOST = (("AMGX_HOST_IMAGES", "1"),)


@functools.lru_cache(maxsize=None)
def _scalar():
    """tridiagonal level (fewer than 3 entries per row: the device builder takes it without a hook) + its blocked colouring"""
    from ngsamg_amd.device import hybrid_gs_data
    H = R.gs_hierarchy(R.long_row_matrix(3, N, seed=1), seed=1)
    color, nc, dinv = hybrid_gs_data(H.levels[0].A, H.levels[0].free, B_SCALAR)
    return H, dict(color=color, n_colors=nc, dinv=dinv, gs_block_rows=B_SCALAR)


@functools.lru_cache(maxsize=None)
def _block():
    """3 x 3 block level, five blocks per row; blocked colouring with a scaled inverse of the diagonal blocks, inv(A_kk) / fac_k with
    fac_k = 1.5 on every third block row (hybrid form: what the l1 modification of the host setup gives on levels that are not
    diagonally dominant), and the block colours of the runs of BB rows with the plain inverse (block-coloured form)"""
    from ngsamg_amd.device import block_colored_gs_data, hybrid_gs_data
    H = R.gs_hierarchy(R.block_long_row_matrix(BS, 5, N, seed=2), bs=BS, seed=2)
    lv = H.levels[0]
    color, nc, _ = hybrid_gs_data(lv.A, lv.free, BB)
    fac = np.where(np.arange(N) % 3 == 0, 1.5, 1.0)
    scaled = np.ascontiguousarray((lv.dinv.reshape(N, BS * BS) / fac[:, None]).reshape(-1))
    c2, nc2, bcol, nbc, plain = block_colored_gs_data(lv.A, lv.free, BB, lv.dinv)
    hybrid = dict(color=color, n_colors=nc, dinv=scaled, gs_block_rows=BB)
    coloured = dict(color=c2, n_colors=nc2, dinv=plain, gs_block_rows=BB, gs_block_color=bcol, gs_n_block_colors=nbc)
    return H, hybrid, coloured


def _create(H, over, monkeypatch, env=()):
    """amgx_create of H (multicolour descriptor) with the fields `over` set on level 0; a DeviceAMGMatrix that owns the handle"""
    from ngsamg_amd import _lib
    from ngsamg_amd.device import DeviceAMGMatrix, hierarchy_desc
    lib = _lib.hip()
    desc, keep, _ = hierarchy_desc(H, "gs")
    d = desc.levels[0]
    for k, v in over.items():
        if isinstance(v, np.ndarray):
            v = np.ascontiguousarray(v)
            keep.append(v)
            v = _lib.ptr(v, C.c_double if v.dtype == np.float64 else C.c_int32)
        setattr(d, k, v)
    h = C.c_void_p()
    with monkeypatch.context() as m:
        for k, v in env:
            m.setenv(k, v)
        rc = lib.amgx_create(C.byref(desc), C.byref(h))
    if rc != 0:
        raise _lib.NgsAMGError(lib.amgx_last_error(None).decode())
    dev = DeviceAMGMatrix.view(h, H)
    dev._owned, dev._keep = True, keep
    return dev


def _changed(over, **arrays):
    """`over` with entries of its arrays replaced: name = (index, value) or a whole array"""
    out = dict(over)
    for k, v in arrays.items():
        if isinstance(v, tuple):
            a = np.array(over[k], copy=True)
            a[v[0]] = v[1]
            v = a
        out[k] = v
    return out


def _mult(dev, H, seed=0):
    n = H.levels[0].A.n_rows * H.levels[0].A.br
    b = np.random.default_rng(seed).standard_normal(n)
    x = np.full(n, np.nan)
    dev.Mult(b, x)
    assert np.isfinite(x).all()
    return x


def _refused(H, valid, bad, message, monkeypatch):
    from ngsamg_amd._lib import NgsAMGError
    with pytest.raises(NgsAMGError) as e:
        _create(H, bad, monkeypatch)
    assert message in str(e.value), str(e.value)
    _mult(_create(H, valid, monkeypatch), H)          # the refusal left the process usable


# ---- refusals ------------------------------------------------------------------------------------------------------------

COUPLED = {"gs": "invalid colouring: two coupled rows share a colour",
           "gsb": "invalid blocked colouring: two coupled rows of one block share a colour",
           "bgsb": "invalid blocked colouring: two coupled block rows of one block share a colour"}


def _builder_input(builder):
    if builder == "gs":
        H = _scalar()[0]
        return H, dict(color=H.levels[0].color, n_colors=H.levels[0].n_colors)
    if builder == "gsb":
        return _scalar()
    return _block()[:2]


@pytest.mark.parametrize("builder", ["gs", "gsb", "bgsb"])
def test_coupled_rows_of_one_unit_sharing_a_colour_are_refused(builder, monkeypatch):
    """rows 0 and 1 are coupled and lie in one block"""
    H, valid = _builder_input(builder)
    _refused(H, valid, _changed(valid, color=(1, valid["color"][0])), COUPLED[builder], monkeypatch)


@pytest.mark.parametrize("builder", ["gs", "gsb", "bgsb"])
def test_colour_index_beyond_n_colors_is_refused(builder, monkeypatch):
    H, valid = _builder_input(builder)
    _refused(H, valid, _changed(valid, color=(5, valid["n_colors"])), "colour index out of range", monkeypatch)


def test_block_ids_are_validated(monkeypatch):
    """gs_block_ids: a block of 22 rows where gs_block_rows is 21; coupled rows of one listed block sharing a colour"""
    H, valid, _ = _block()
    runs = (np.arange(N) // BB).astype(np.int32)
    valid = dict(valid, gs_block_ids=runs)
    _refused(H, valid, dict(valid, gs_block_ids=(np.arange(N) // (BB + 1)).astype(np.int32)),
             "gs_block_ids: a block has more than gs_block_rows rows", monkeypatch)
    _refused(H, valid, _changed(valid, color=(1, valid["color"][0])),
             "invalid blocked colouring: two coupled block rows of one sweep block share a colour", monkeypatch)


def test_block_colours_are_validated(monkeypatch):
    """gs_block_color: not constant inside a sweep block; two coupled sweep blocks (0 and 1) of one block colour"""
    H, _, valid = _block()
    bcol = valid["gs_block_color"]
    assert valid["gs_n_block_colors"] >= 2 and bcol[0] != bcol[BB]
    _refused(H, valid, _changed(valid, gs_block_color=(1, bcol[BB])), "gs_block_color: not constant inside a sweep block", monkeypatch)
    _refused(H, valid, dict(valid, gs_block_color=np.zeros(N, np.int32)),
             "invalid block colouring: two coupled sweep blocks share a colour", monkeypatch)


# ---- branches on which the split images are declined, device builder against host builder ---------------------------------

def _both_builders(H, over, monkeypatch, form, split):
    dv, hs = _create(H, over, monkeypatch, DEVICE), _create(H, over, monkeypatch, HOST)
    lp = dv.level_paths(0)
    assert lp == hs.level_paths(0)
    assert lp["gs_form"] == form and lp["gs_split"] == split, lp
    assert np.array_equal(_mult(dv, H), _mult(hs, H))


def test_scalar_hybrid_swept_row_without_diagonal_inverse_declines_the_split(monkeypatch):
    """a swept row whose dinv is 0: cvec = 1 / dinv - a_kk does not exist, both builders keep the sweep over the whole image"""
    H, valid = _scalar()
    assert valid["color"][7] >= 0
    _both_builders(H, valid, monkeypatch, "hybrid", 1)
    _both_builders(H, _changed(valid, dinv=(7, 0.0)), monkeypatch, "hybrid", 0)


def test_block_coloured_level_with_a_scaled_inverse_declines_the_split(monkeypatch):
    """the block-coloured form expects the plain inverse of the diagonal blocks (fac = 1); with a scaled one (fac = 1.5 on every third
    block row) both builders keep sweep + full residual, while the hybrid form takes it (its rest image carries fac - 1)"""
    H, hybrid, coloured = _block()
    A = H.levels[0].A.to_scipy().toarray().reshape(N, BS, N, BS)
    m00 = np.array([(hybrid["dinv"].reshape(N, BS, BS)[k] @ A[k, :, k, :])[0, 0] for k in range(N)])
    assert np.allclose(m00[0::3], 1.0 / 1.5) and np.allclose(m00[1::3], 1.0)          # Dinv_k A_kk = I / fac_k
    _both_builders(H, coloured, monkeypatch, "block-coloured", 1)
    _both_builders(H, dict(coloured, dinv=hybrid["dinv"]), monkeypatch, "block-coloured", 0)
    _both_builders(H, hybrid, monkeypatch, "hybrid-block", 1)


def test_rank_without_rows_device_builder_equals_host_builder(monkeypatch):
    """two virtual ranks, the first owns nothing: its levels have no rows (the hybrid form is "on" there with no block to sweep, by the
    host side of the builder whatever the hooks say), the other rank's images come from the device kernels / the host loops
    (AMGX_SELL_MAX_LANES=1: the one-lane images the device builder forms, on both sides)"""
    import scipy.sparse as sp
    import torch
    from ngsamg_amd import bridge as B, dist as D

    def cycle(env):
        comm = D.LoopbackComm(2)
        L, _ = B.shared_poisson_partition(0, (1, 1, 1), (17, 17, 9))
        L.rank = 1
        L.dist_procs = [np.asarray(p) + 1 for p in L.dist_procs]
        empty = B.SharedLocal(0, sp.csr_matrix((0, 0)), [], free=np.zeros(0, dtype=np.uint8), coords=np.zeros((0, 3)))
        states = B.from_shared_layout(comm, [empty, L])[0]
        assert states[0].n == 0 and states[1].n > 0
        with monkeypatch.context() as m:
            for k, v in env + (("AMGX_SELL_MAX_LANES", "1"),):
                m.setenv(k, v)
            amg = D.DistributedAMG(comm, states, dim=3, dist_min_rows=60, device=0, max_coarse_size=10, sm_type="hgs", hgs_block_rows=256,
                                   gs_stage_min_rows=50)
        assert amg.k >= 1
        paths = [[o.top.level_paths(l) for l in range(amg.k)] for o in amg._dev.ops]
        rng = np.random.default_rng(1)
        bs = [torch.from_numpy(rng.standard_normal(s.n) * s.free).cuda() for s in states]
        xs = [torch.full((s.n,), float("nan"), dtype=torch.float64, device="cuda") for s in states]
        amg.Mult(bs, xs)
        torch.cuda.synchronize()
        return paths, xs[1].cpu().numpy()

    pd, xd = cycle(DEVICE)
    ph, xh = cycle(HOST)
    assert pd == ph and pd[1][0]["gs_form"] == "hybrid" and pd[1][0]["gs_split"] == 1, pd
    assert pd[0][0]["gs_split"] == 0, pd[0][0]
    assert np.isfinite(xd).all() and np.array_equal(xd, xh)
