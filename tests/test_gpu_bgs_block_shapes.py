"""Every instantiation of bgs_block_kernel<BS, TH, G> (block Gauss-Seidel over aggregate blocks) that the host rule
bgs_block_shape (amgx.hip) can pick, for BS = 1, 2, 3, 6, on hand-made single levels through the C ABI, against a plain numpy
sweep.  The hierarchies of the parity tests have blocks of at most 48 scalar dofs and reach <256, 4> and <1024, 16> only.

The rule: G = 4 for levels with at most 30 blocks per row, else 16 while the largest block has max_m <= 64 scalar dofs, else 8;
TH = 256 / 512 / 1024 from max_m * 4 for G = 4, and 1024 for G = 8 and 16.  Reachable (TH, G) and what a block of M scalar dofs
meets inside the kernel (S = TH / M slices of the inverse, held in registers while ceil(M / S) <= 16, else read from memory in
the second phase; the row loop takes ceil(M * G / TH) passes):

  (TH, G)      level                      blocks M (BS = 1; multiples of BS near them otherwise)
  <256, 4>     avg <= 30, max_m <= 64     BS, 40, 64 (S = 4: exactly 16 entries per thread)
  <512, 4>     avg <= 30, max_m <= 128    BS, 65 (registers), 90 (S = 5: memory), 128 (one pass exactly)
  <1024, 4>    avg <= 30, max_m > 128     BS, 7 BS, 129, 256 (one pass exactly), 300 (two passes), 1024 (four passes; 1023, 1020)
  <1024, 16>   avg > 30, max_m <= 64      BS, 30, 64 (one pass exactly)
  <1024, 8>    avg > 30, max_m > 64       128 (one pass exactly, registers), 130 (two passes, memory), 600 (five passes)

Unreachable by construction, hence not tested: <512, 8> (G = 8 means max_m > 64, so max_m * 8 > 512; the dispatcher has no such
line), and the kernel's `!fits` branch (M > TH): TH >= max_m for every admitted block, since amgx_create refuses blocks of more
than 1024 scalar dofs (test_block_beyond_1024_dofs_is_refused).

Every case asserts the (TH, G, max_m) the device reports through level_paths ("bgs_threads", "bgs_lanes", "bgs_max_m": the value
of the function the dispatcher calls, not a restatement), then runs Smooth forward and backward from a random x and forward from
zero.  Reference: the colours in the device's order (ascending forward, descending backward; blocks of one colour are not
coupled), per block x_B += solve(A_BB, b_B - A_B: x) with numpy.linalg.solve on A_BB itself -- not the handed-over inverse --
and the row products accumulated in long double.  Tolerance 1e-10 relative (Gauss-Seidel in the GPU's own
order); the handed-over inverses agree with solve to 1.5e-14 on these matrices."""
import functools

import numpy as np
import pytest

from ngsamg_amd._lib import Matrix, NgsAMGError
from ngsamg_amd.hierarchy import BGSData, Level, bgs_data
from tests import reorder as R

pytestmark = pytest.mark.gpu

LD = np.longdouble


# name: (TH, G, half band in vertices, blocks).  A block is (M, how): M scalar dofs for BS = 1 and, for the other block sizes,
# "v" M vertices, "d" / "u" the nearest multiple of BS below / above M (whichever keeps the block on its side of the thresholds)
SHAPES = {
    "256x4": (256, 4, 3, ((1, "v"), (40, "d"), (64, "d"))),
    "512x4": (512, 4, 3, ((1, "v"), (65, "u"), (90, "d"), (128, "d"))),
    "1024x4": (1024, 4, 3, ((1, "v"), (7, "v"), (129, "u"), (256, "d"), (300, "d"), (1024, "d"))),
    "1024x16": (1024, 16, 16, ((1, "v"), (30, "d"), (64, "d"))),
    "1024x8": (1024, 8, 16, ((128, "d"), (130, "u"), (600, "d"))),
}
MIN_VERTICES = 600          # (also keeps the average of the 33-block rows above 30: 33 - 16 * 17 / n)


def _sizes(name, bs):
    """block sizes (scalar dofs, multiples of bs) of one level"""
    return [M * bs if how == "v" else (M // bs) * bs if how == "d" else -(-M // bs) * bs for M, how in SHAPES[name][3]]


class _H:
    def __init__(self, levels):
        self.levels = levels
        self.coarse_n = 0
        self.coarse_inv = np.empty(0)
        self.n_levels = len(levels)


def _level(A, bs, g):
    n = A.n_rows
    return Level(A=A, P=None, PT=None, free=np.ones(n, dtype=np.uint8), dinv=np.tile(np.eye(bs).reshape(-1), n), coords=None,
                 color=np.full(n, -1, dtype=np.int32), n_colors=0, agg=None, bgs=g)


@functools.lru_cache(maxsize=None)
def _case(name, bs):
    """(scipy A, Matrix, BGSData, sizes): a banded, strictly diagonally dominant SPD matrix with bs x bs blocks
    (reorder.block_long_row_matrix: 2 hb + 1 blocks in the longest row) and consecutive vertex ranges of the listed sizes as blocks,
    the list repeated: every size occurs at least twice and the level has at least MIN_VERTICES vertices"""
    hb = SHAPES[name][2]
    sizes = _sizes(name, bs)
    per = sum(M // bs for M in sizes)
    verts = [M // bs for M in sizes] * max(2, -(-MIN_VERTICES // per))
    n = int(sum(verts))
    A = R.block_long_row_matrix(bs, 2 * hb + 1, n, seed=bs + 10 * hb)
    m = Matrix.from_scipy(A, bs) if bs > 1 else Matrix.from_scipy(A)
    ptr = np.concatenate([[0], np.cumsum(verts)]).astype(np.int32)
    g = bgs_data(m, ptr, np.arange(n, dtype=np.int32), pinv=False)
    return A, m, g, sizes


def _reference(A, bs, g, x0, b, back):
    """one sweep, colour by colour, solve() on the diagonal blocks, long double accumulation"""
    x = np.asarray(x0, dtype=LD).copy()
    colors = range(g.n_colors - 1, -1, -1) if back else range(g.n_colors)
    data = A.data.astype(LD)
    for c in colors:
        for k in np.nonzero(g.color == c)[0]:
            rows = g.block_rows[g.block_ptr[k]:g.block_ptr[k + 1]]
            r0, r1 = int(rows[0]) * bs, (int(rows[-1]) + 1) * bs          # consecutive vertices
            lo, hi = A.indptr[r0], A.indptr[r1]
            prod = data[lo:hi] * x[A.indices[lo:hi]]
            r = b[r0:r1].astype(LD) - np.add.reduceat(prod, A.indptr[r0:r1] - lo)       # (every row has its diagonal: no empty row)
            ABB = A[r0:r1, r0:r1].toarray()
            x[r0:r1] += np.linalg.solve(ABB, r.astype(np.float64))
    return x


@pytest.mark.parametrize("bs", [1, 2, 3, 6])
@pytest.mark.parametrize("name", list(SHAPES))
def test_bgs_block_kernel_shapes(name, bs):
    from ngsamg_amd.device import DeviceAMGMatrix
    TH, G = SHAPES[name][:2]
    A, m, g, sizes = _case(name, bs)
    n = A.shape[0]
    avg = m.nnz / m.n_rows
    assert (avg > 30.0) == (G != 4), avg                 # the level is on the side of the threshold the case is about
    dev = DeviceAMGMatrix(_H([_level(m, bs, g)]), sm_type="bgs", clev="none", device=0)
    lp = dev.level_paths(0)
    assert lp["gs_form"] == "bgs" and lp["gs_colors"] == g.n_colors, lp
    assert (lp["bgs_threads"], lp["bgs_lanes"], lp["bgs_max_m"]) == (TH, G, max(sizes)), (lp, sizes)
    rng = np.random.default_rng(1000 * bs + TH + G)
    for back, zero in ((False, False), (True, False), (False, True)):
        b = rng.standard_normal(n)
        x0 = np.zeros(n) if zero else rng.standard_normal(n)
        xg, res = x0.copy(), np.zeros(n)
        dev.Smooth(0, xg, b, res, False, False, zero, back=back)
        ref = _reference(A, bs, g, x0, b, back)
        err = float(np.linalg.norm(xg - ref) / np.linalg.norm(ref))
        print(f"{name} bs={bs} M={sizes} colours={g.n_colors} back={back} zero={zero}: rel.err {err:.2e}")
        assert err <= 1e-10, (name, bs, back, zero, err)
        # per block, so that one wrong small block cannot hide behind the norm of the large ones
        for k in range(g.n_blocks):
            r0, r1 = g.block_ptr[k] * bs, g.block_ptr[k + 1] * bs
            ek = float(np.linalg.norm(xg[r0:r1] - ref[r0:r1]) / max(np.linalg.norm(ref[r0:r1]), np.linalg.norm(ref) / np.sqrt(n)))
            assert ek <= 1e-10, (name, bs, back, zero, k, int(r1 - r0), ek)


def test_block_beyond_1024_dofs_is_refused():
    """amgx_create refuses a block of more than 1024 scalar dofs (the kernel's LDS arrays hold 1024): an error return"""
    from ngsamg_amd.device import DeviceAMGMatrix
    n = 1025
    A = R.long_row_matrix(7, n)
    m = Matrix.from_scipy(A)
    g = BGSData(1, np.array([0, n], dtype=np.int32), np.arange(n, dtype=np.int32), np.array([0, n * n], dtype=np.int64),
                np.zeros(n * n), np.zeros(1, dtype=np.int32), 1)
    with pytest.raises(NgsAMGError, match="block with more than 1024 scalar dofs"):
        DeviceAMGMatrix(_H([_level(m, 1, g)]), sm_type="bgs", clev="none", device=0)


def test_level_paths_fills_its_documented_entries_and_no_more():
    """the C entry point writes min(n_out, AMGX_LEVEL_PATHS_N = 40) values: a longer buffer keeps its tail, a shorter one is not overrun"""
    from ngsamg_amd import _lib
    from ngsamg_amd.device import DeviceAMGMatrix
    A, m, g, sizes = _case("256x4", 1)
    dev = DeviceAMGMatrix(_H([_level(m, 1, g)]), sm_type="bgs", clev="none", device=0)
    N = len(DeviceAMGMatrix._PATH_KEYS)
    full = np.full(N + 8, -7, dtype=np.int64)
    assert dev._lib.amgx_level_paths(dev._h, 0, full.ctypes.data_as(_lib.c_i64p), full.size) == 0
    assert np.all(full[N:] == -7) and tuple(full[34:37]) == (256, 4, 64) and np.all(full[37:N] == 0)
    short = np.full(N, -7, dtype=np.int64)
    assert dev._lib.amgx_level_paths(dev._h, 0, short.ctypes.data_as(_lib.c_i64p), 36) == 0
    assert np.array_equal(short[:36], full[:36]) and np.all(short[36:] == -7)
