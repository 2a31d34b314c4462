"""Grid recognition and box chunks of the diagonal image (amgh_dia_grid / amgh_dia_boxes / amgh_dia_box_neighbours, host/dia.hpp):
the code amgx_create runs to cut a lexicographic grid level into boxes of whole grid lines, and the local-index arithmetic
dia_box_pre_restrict_kernel shares with it."""
import ctypes as C

import numpy as np
import pytest

from ngsamg_amd import _lib

GRIDS = [(70, 5, 6), (9, 9, 9), (130, 7), (215, 3, 5)]


def _i32(v):
    return np.ascontiguousarray(v, dtype=np.int32)


def kuhn_offsets(shape):
    nx = shape[0]
    if len(shape) == 2:
        return [1, nx, nx + 1]
    s = nx * shape[1]
    return [1, nx, nx + 1, s, s + 1, s + nx, s + nx + 1]


def grid(n, offs):
    o = _i32(offs)
    shape = np.zeros(3, dtype=np.int64)
    d = np.full(3 * max(len(offs), 1), -1, dtype=np.int32)
    _lib.hcheck(_lib.host().amgh_dia_grid(n, len(offs), o.ctypes.data_as(_lib.c_i32p), shape.ctypes.data_as(_lib.c_i64p), d.ctypes.data_as(_lib.c_i32p)))
    return tuple(int(v) for v in shape), [tuple(int(v) for v in d[3 * k:3 * k + 3]) for k in range(len(offs))]


def boxes(n, offs, yc=0, zc=0):
    """(yc, zc, run_ptr, first, len) or None when the grid takes no boxes"""
    o = _i32(offs)
    cnt = np.zeros(4, dtype=np.int64)
    f = _lib.host().amgh_dia_boxes
    _lib.hcheck(f(n, len(offs), o.ctypes.data_as(_lib.c_i32p), yc, zc, cnt.ctypes.data_as(_lib.c_i64p), None, None, None))
    if cnt[0] == 0:
        return None
    rp, first, ln = np.zeros(cnt[0] + 1, dtype=np.int64), np.zeros(cnt[1], dtype=np.int64), np.zeros(cnt[1], dtype=np.int32)
    _lib.hcheck(f(n, len(offs), o.ctypes.data_as(_lib.c_i32p), yc, zc, cnt.ctypes.data_as(_lib.c_i64p), rp.ctypes.data_as(_lib.c_i64p),
                  first.ctypes.data_as(_lib.c_i64p), ln.ctypes.data_as(_lib.c_i32p)))
    return int(cnt[2]), int(cnt[3]), rp, first, ln


def neighbours(n, offs, box, k, up, rows, yc=0, zc=0):
    o = _i32(offs)
    out = np.full(rows, -7, dtype=np.int32)
    _lib.hcheck(_lib.host().amgh_dia_box_neighbours(n, len(offs), o.ctypes.data_as(_lib.c_i32p), yc, zc, box, k, int(up), out.ctypes.data_as(_lib.c_i32p)))
    return out


@pytest.mark.parametrize("shape", GRIDS)
def test_kuhn_offsets_decompose(shape):
    n = int(np.prod(shape))
    offs = kuhn_offsets(shape)
    got, d = grid(n, offs)
    assert got == (tuple(shape) + (1,))[:3]
    sy, sz = shape[0], shape[0] * shape[1]
    assert [dx + dy * sy + dz * sz for dx, dy, dz in d] == offs
    assert all(v in (0, 1) for t in d for v in t) and (len(shape) == 3 or all(t[2] == 0 for t in d))


def test_seven_point_offsets_decompose():
    nx, ny, nz = 41, 37, 29
    got, d = grid(nx * ny * nz, [1, nx, nx * ny])
    assert got == (nx, ny, nz) and d == [(1, 0, 0), (0, 1, 0), (0, 0, 1)]
    got, d = grid(130 * 110, [1, 130])
    assert got == (130, 110, 1) and d == [(1, 0, 0), (0, 1, 0)]


def test_refusals():
    nx, ny, nz = 41, 37, 29
    n = nx * ny * nz
    assert grid(n + 1, kuhn_offsets((nx, ny, nz)))[0] == (0, 0, 0)           # n is no multiple of sz
    assert grid(130 * 110 + 3, [1, 130, 131])[0] == (0, 0, 0)               # 2D: n is no multiple of sy
    assert grid(130 * 110, [1, 129, 130, 131])[0] == (0, 0, 0)              # the 9-point stencil's nx - 1
    assert grid(n, [1, nx, nx + 1, nx * ny - 1])[0] == (0, 0, 0)            # sz = nx ny - 1 is no multiple of sy
    assert grid(n, [1, nx, nx * ny, nx * ny + 2])[0] == (0, 0, 0)           # dx = 2
    assert grid(20000, [1])[0] == (0, 0, 0)                                 # fewer than two offsets
    assert grid(20000, [2, 100])[0] == (0, 0, 0)                            # no x neighbour
    assert grid(20000, [1, 3, 64, 65, 500])[0] == (0, 0, 0)
    # a line of 5 rows: a full 2 x 4 box has 40 rows, less than 3/4 of one wave
    assert grid(5 * 6 * 7, kuhn_offsets((5, 6, 7)))[0] == (5, 6, 7) and boxes(5 * 6 * 7, kuhn_offsets((5, 6, 7))) is None
    # a line longer than a box may be
    assert boxes(3000 * 4, kuhn_offsets((3000, 4))) is None


@pytest.mark.parametrize("shape", GRIDS)
def test_boxes_cover_every_row_once_in_whole_clipped_lines(shape):
    n = int(np.prod(shape))
    offs = kuhn_offsets(shape)
    nx, ny = shape[0], shape[1]
    nz = shape[2] if len(shape) == 3 else 1
    yc, zc, rp, first, ln = boxes(n, offs)
    assert (yc, zc) == ((2, 4) if len(shape) == 3 else (8, 1))
    # whole lines, every row in exactly one run
    assert np.all(ln == nx) and np.all(first % nx == 0)
    cover = np.zeros(n, dtype=np.int64)
    for f, l in zip(first, ln):
        cover[f:f + l] += 1
    assert np.all(cover == 1)
    # boxes numbered y fastest, then z; clipped at the edges, never padded; lines of a box y fastest, then z
    nby, nbz = -(-ny // yc), -(-nz // zc)
    assert len(rp) == nby * nbz + 1
    for c in range(nby * nbz):
        by, bz = c % nby, c // nby
        ys = range(by * yc, min(ny, (by + 1) * yc))
        zs = range(bz * zc, min(nz, (bz + 1) * zc))
        want = [(z * ny + y) * nx for z in zs for y in ys]
        assert list(first[rp[c]:rp[c + 1]]) == want
    assert max(np.diff(rp)) == min(yc, ny) * min(zc, nz)


@pytest.mark.parametrize("shape", GRIDS)
@pytest.mark.parametrize("yz", [(0, 0), (2, 2), (1, 4)])
def test_neighbour_local_index_is_the_position_in_the_run_list(shape, yz):
    n = int(np.prod(shape))
    offs = kuhn_offsets(shape)
    _, d = grid(n, offs)
    b = boxes(n, offs, *yz)
    if b is None:                                # (9, 9, 9) in 2 x 2 or 1 x 4 lines: 36 rows, less than 3/4 of one wave
        assert shape[0] * yz[0] * yz[1] < 48
        return
    if len(shape) == 2 and yz != (0, 0):
        assert b[1] == 1                         # 2D: one plane
    yc, zc, rp, first, ln = b
    pos_box = np.full(n, -1, dtype=np.int64)     # box and position in the box's run list of every row
    pos_loc = np.full(n, -1, dtype=np.int64)
    for c in range(len(rp) - 1):
        rows = np.concatenate([np.arange(f, f + l) for f, l in zip(first[rp[c]:rp[c + 1]], ln[rp[c]:rp[c + 1]])])
        pos_box[rows] = c
        pos_loc[rows] = np.arange(rows.size)
    for c in range(len(rp) - 1):
        rows = np.flatnonzero(pos_box == c)
        rows = rows[np.argsort(pos_loc[rows])]
        for k, o in enumerate(offs):
            for up in (False, True):
                j = rows + o if up else rows - o
                ok = (j >= 0) & (j < n)
                want = np.full(rows.size, -1, dtype=np.int64)
                same = ok.copy()
                same[ok] = pos_box[j[ok]] == c
                want[same] = pos_loc[j[same]]
                got = neighbours(n, offs, c, k, up, rows.size, *yz)
                # every local index is the position in the run list (also for x + dx = nx, where row + o_k is the first vertex
                # of the next line); the only in-box rows answered with -1 -- the kernel then reads their operands from global
                # memory, the same bits -- are steps that leave the grid plane in y and re-enter the box through the next plane
                assert np.array_equal(got[got >= 0], want[got >= 0]), (c, k, up)
                dx, dy, _ = d[k]
                x, y = rows % shape[0], (rows // shape[0]) % shape[1]
                wrapped = (y + dy + (x + dx >= shape[0]) >= shape[1]) if up else (y - dy - (x - dx < 0) < 0)
                assert np.array_equal(got < 0, (want < 0) | wrapped), (c, k, up)
