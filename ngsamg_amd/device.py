"""Device-resident AMG matrix: Python handle over the C ABI of include/amgx.h.

Mirrors the reference's ``AMGMatrix`` (reference src/base/solve/amg_matrix.hpp:14-87, pybind surface
src/base/solve/python_solve.cpp:55-109): ``Mult`` / ``MultAdd`` run one multigrid cycle, ``GetSmoother(level)``
exposes ``Smooth`` / ``SmoothBack`` with the reference's flag contract, ``GetMap()`` the grid transfers.

Vectors may be numpy arrays (host: one H2D and one D2H copy per call, like a CPU caller of the reference)
or torch CUDA tensors (device resident: no copies; the work is enqueued on torch's current stream).
There is no CPU fallback: without the HIP library or without a GPU, construction raises.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import Matrix, NgsAMGError

# "hgs" = Gauss-Seidel in the block-hybrid form (one launch per sweep, amgx_level_desc.gs_block_rows); "gs" = multicolour
# "cheby" = Chebyshev polynomial smoother in the (block-)Jacobi-preconditioned operator (an own option)
_SM = {"jacobi": _lib.AMGX_SM_JACOBI, "gs": _lib.AMGX_SM_GS, "hgs": _lib.AMGX_SM_GS, "bgs": _lib.AMGX_SM_BGS,
       "cheby": _lib.AMGX_SM_CHEBY}


def _per_level(v, i, n, name):
    """scalar or per-level list"""
    if isinstance(v, (list, tuple, np.ndarray)):
        if len(v) != n:
            raise NgsAMGError(f"{name} list must have one entry per level")
        return v[i]
    return v


def cheby_args(degree, ratio, lambda_max, i=0, n=1):
    """validated (degree, lambda_max, ratio) of one Chebyshev level as the descriptor carries them (0 = default / estimate)"""
    deg = _per_level(degree, i, n, "cheb_degree")
    rat = _per_level(ratio, i, n, "cheb_ratio")
    lam = _per_level(lambda_max, i, n, "cheb_lambda_max")
    deg = 2 if deg is None else int(deg)
    rat = 10.0 if rat is None else float(rat)
    lam = 0.0 if lam is None else float(lam)
    if not (1 <= deg <= 8):
        raise NgsAMGError(f"cheb_degree = {deg}: need 1 .. 8")
    if not (rat > 1.0):
        raise NgsAMGError(f"cheb_ratio = {rat}: need a ratio > 1")
    if not (lam >= 0.0):
        raise NgsAMGError(f"cheb_lambda_max = {lam}: need a value >= 0 (0 / None: estimated on the device)")
    return deg, lam, rat


_PREC = {"double": _lib.AMGX_PREC_F64, "single": _lib.AMGX_PREC_F32, "single_gs": _lib.AMGX_PREC_F32, "single_gs_all": _lib.AMGX_PREC_F32_SCALAR_GS}
# the smoother types a value of mat_prec applies to
_PREC_TYPES = {"single": ("cheby",), "single_gs": ("cheby", "gs", "hgs"), "single_gs_all": ("cheby", "gs", "hgs")}


def mat_prec_levels(mat_prec, types):
    """amgx_level_desc.mat_prec of every level for the smoother types `types` (one per level, the last = the coarsest, which
    ignores the field).  mat_prec: "double", "single", "single_gs", "single_gs_all" or a per-level list of them.  A scalar "single" applies to the
    Chebyshev levels and needs at least one; a list may say "single" on Chebyshev levels only.  "single_gs"
    applies to the Chebyshev and the Gauss-Seidel ("gs", "hgs") levels in the same way (on a Gauss-Seidel level
    the images of the block sweeps; a level whose sweep form has none stays fp64).  "single_gs_all" = "single_gs" + the scalar
    Gauss-Seidel levels: AMGX_PREC_F32_SCALAR_GS (2) on "gs" / "hgs" levels -- hierarchy_desc turns it into
    AMGX_PREC_F32 where the level has blocks -- and AMGX_PREC_F32 (1) on "cheby" levels."""
    n = len(types)
    per_level = isinstance(mat_prec, (list, tuple))
    vals = list(mat_prec) if per_level else [mat_prec] * n
    if len(vals) != n:
        raise NgsAMGError("mat_prec list must have one entry per level")
    for v in vals:
        if not isinstance(v, str) or v not in _PREC:
            raise NgsAMGError(f"unknown mat_prec {v!r} (double | single | single_gs | single_gs_all)")
    out = [0] * n
    for i in (range(n - 1) if n > 1 else range(n)):       # smoothed levels (a single level: a stand-alone smoother)
        if vals[i] == "double":
            continue
        if types[i] in _PREC_TYPES[vals[i]]:
            out[i] = _lib.AMGX_PREC_F32_SCALAR_GS if vals[i] == "single_gs_all" and types[i] in ("gs", "hgs") else _lib.AMGX_PREC_F32
        elif per_level and vals[i] == "single":
            raise NgsAMGError(f"mat_prec 'single' on level {i}: single-precision matrix storage is available on Chebyshev "
                              f"levels only (sm_type '{types[i]}')")
        elif per_level:
            raise NgsAMGError(f"mat_prec '{vals[i]}' on level {i}: single-precision matrix storage is available on Chebyshev and "
                              f"Gauss-Seidel levels only (sm_type '{types[i]}')")
    if not per_level and mat_prec == "single" and not any(out):
        raise NgsAMGError("mat_prec 'single': the hierarchy has no Chebyshev level (sm_type 'cheby') to apply it to")
    if not per_level and mat_prec in ("single_gs", "single_gs_all") and not any(out):
        raise NgsAMGError(f"mat_prec '{mat_prec}': the hierarchy has no Chebyshev or Gauss-Seidel level (sm_type 'cheby', 'gs', 'hgs') "
                          "to apply it to")
    return out


_JPREC = {"double": _lib.AMGX_JACOBI_PREC_F64, "single": _lib.AMGX_JACOBI_PREC_F32, "single_wide": _lib.AMGX_JACOBI_PREC_F32_WIDE}


def jacobi_prec_levels(jacobi_prec, types, block_sizes=None):
    """amgx_level_desc.jacobi_prec of every level for the smoother types `types` and the block sizes of the level
    matrices (one each per level, the last = the coarsest, which ignores the field; block_sizes None: all scalar).  jacobi_prec:
    "double", "single", "single_wide" (the A/B twin: rounded values at fp64 width) or a per-level list of them.  A scalar request
    applies to the scalar Jacobi levels and needs at least one; a list may name such levels only."""
    n = len(types)
    bs = list(block_sizes) if block_sizes is not None else [1] * n
    per_level = isinstance(jacobi_prec, (list, tuple))
    vals = list(jacobi_prec) if per_level else [jacobi_prec] * n
    if len(vals) != n or len(bs) != n:
        raise NgsAMGError("jacobi_prec list must have one entry per level")
    for v in vals:
        if not isinstance(v, str) or v not in _JPREC:
            raise NgsAMGError(f"unknown jacobi_prec {v!r} (double | single | single_wide)")
    out = [0] * n
    for i in (range(n - 1) if n > 1 else range(n)):       # smoothed levels (a single level: a stand-alone smoother)
        if vals[i] == "double":
            continue
        if types[i] == "jacobi" and bs[i] == 1:
            out[i] = _JPREC[vals[i]]
        elif per_level:
            raise NgsAMGError(f"jacobi_prec '{vals[i]}' on level {i}: single-precision Jacobi images are available on scalar Jacobi "
                              f"levels only (sm_type '{types[i]}', block size {bs[i]})")
    if not per_level and jacobi_prec != "double" and not any(out):
        raise NgsAMGError(f"jacobi_prec '{jacobi_prec}': the hierarchy has no scalar Jacobi level (sm_type 'jacobi', block size 1) "
                          "to apply it to")
    return out


def gs_block_rows(A):
    """rows per block of the block-hybrid Gauss-Seidel kernel for a scalar level matrix.  G lanes share a row, each holds
    at most 16 entries (+1 when G = 1) in registers; the workgroup has B * G lanes.  Measured at cfg 2:
    one-lane rows run fastest in 256-row blocks (more workgroups per CU hide the colour phases of their neighbours); rows
    that need several lanes get 512-lane workgroups (1024 until round 3).
    0: the level keeps the multicolour form (rows too long, or a level small enough for the single-workgroup tail)."""
    import os
    if A.br == A.bc and A.br in (2, 3, 6) and A.n_rows == A.n_cols:
        # square-block levels (bgsb_sweep_kernel): a workgroup owns ~128 block rows, a whole number of BSELL slices
        # (64 // bs block rows each); levels with fewer than four such blocks keep the multicolour form
        # (levels below 50 k block rows are latency-bound: a workgroup walks its colour phases one after the other, and half-size
        #  blocks have fewer in-block colours -- A/B at cfg 5, 8 k-row level: 110 + 158 us -> 90 + 101 us per cycle)
        rb = 64 // A.br
        B = int(os.environ.get("AMGX_BGSB_ROWS", "0")) or rb * max(1, (128 if A.n_rows >= 50000 else 64) // rb)
        return B if (A.n_rows >= 4 * B and not os.environ.get("AMGX_NO_BGSB")) else 0
    if A.br != 1 or A.bc != 1 or A.n_rows <= 256:
        return 0
    mx = int(np.diff(A.rowptr).max()) if A.n_rows else 0
    for G in (1, 2, 4, 8, 16):
        if mx <= 16 * G + (1 if G == 1 else 0):
            # (several lanes per row: 512-lane workgroups since round 4 -- on the long-row coarse levels of a reference-shaped hierarchy
            #  one 1024-lane workgroup fills a CU's registers and nothing hides its colour phases: level 1 of cfg 2, backward sweep
            #  299 -> 240 us; PCG iterations at 100^3 with 128 / 64 / 32-row blocks on those levels: 17 / 17 / 17, sequential order 15)
            threads = int(os.environ.get("AMGX_GSB_THREADS", "256") if G == 1 else os.environ.get("AMGX_GSB_THREADS_MULTI", "512"))
            threads = threads if threads in (256, 512, 1024) else 1024
            return max(16, threads // G)
    return 0


def hybrid_gs_data(A, free, B, pinv=False):
    """blocked colouring + inverse of the l1-modified (block) diagonal for blocks of B consecutive rows (host library);
    pinv: block levels whose diagonal blocks are pseudo-inverted (ngs_amg_regularize_cmats)"""
    lib = _lib.host()
    d = A.desc()
    fr = None if free is None else np.ascontiguousarray(free, dtype=np.uint8)
    color = np.full(A.n_rows, -1, dtype=np.int32)
    nc = C.c_int32()
    _lib.hcheck(lib.amgh_coloring_blocked(C.byref(d), _lib.ptr(fr, C.c_uint8), int(B), _lib.ptr(color, C.c_int32), C.byref(nc)))
    if A.br > 1:
        dinv = np.zeros(A.n_rows * A.br * A.br, dtype=np.float64)
        _lib.hcheck(lib.amgh_hybrid_dinv_block(C.byref(d), _lib.ptr(fr, C.c_uint8), int(B), int(bool(pinv)), _lib.ptr(dinv, C.c_double)))
        return color, int(nc.value), dinv
    dinv = np.zeros(A.n_cols, dtype=np.float64)          # (rank-partitioned levels: entries of the ghost columns stay 0)
    _lib.hcheck(lib.amgh_hybrid_dinv(C.byref(d), _lib.ptr(fr, C.c_uint8), int(B), _lib.ptr(dinv, C.c_double)))
    return color, int(nc.value), dinv


def block_colored_gs_data(A, free, B, dinv_plain):
    """square-block levels, block-COLOURED Gauss-Seidel (amgx_level_desc.gs_block_color): sweep blocks = runs of B consecutive block
    rows; in-block colouring as for the hybrid form (amgh_coloring_blocked), a colouring of the BLOCK graph (amgh_bgs_coloring: coupled
    blocks differ) and the plain (pseudo-)inverse of the diagonal blocks -- the sweep is exact Gauss-Seidel in the order (block colour,
    block, in-block colour), so no l1 modification.  Returns (color, n_colors, block_color_of_row, n_block_colors, dinv)."""
    lib = _lib.host()
    d = A.desc()
    fr = None if free is None else np.ascontiguousarray(free, dtype=np.uint8)
    n = A.n_rows
    color = np.full(n, -1, dtype=np.int32)
    nc = C.c_int32()
    _lib.hcheck(lib.amgh_coloring_blocked(C.byref(d), _lib.ptr(fr, C.c_uint8), int(B), _lib.ptr(color, C.c_int32), C.byref(nc)))
    nb = (n + B - 1) // B
    bptr = np.minimum(np.arange(nb + 1, dtype=np.int64) * B, n).astype(np.int32)
    brows = np.arange(n, dtype=np.int32)
    bcol = np.zeros(max(1, nb), dtype=np.int32)
    nbc = C.c_int32()
    _lib.hcheck(lib.amgh_bgs_coloring(C.byref(d), int(nb), _lib.ptr(bptr, C.c_int32), _lib.ptr(brows, C.c_int32), _lib.ptr(bcol, C.c_int32), C.byref(nbc)))
    row_bcol = np.ascontiguousarray(np.repeat(bcol[:nb], B)[:n].astype(np.int32))
    return color, int(nc.value), row_bcol, int(nbc.value), np.ascontiguousarray(dinv_plain, dtype=np.float64)


def hybrid_gs_data_compact(A, free, B, pinv=False):
    """square-block levels: compact sweep blocks of at most B block rows grown over the matrix graph (amgh_compact_blocks)
    instead of runs of consecutive rows, with their colouring and l1-modified block diagonal.
    Returns (block_of_row, color, n_colors, dinv)."""
    lib = _lib.host()
    d = A.desc()
    fr = np.ascontiguousarray(np.ones(A.n_rows, dtype=np.uint8) if free is None else free, dtype=np.uint8)
    blk = np.zeros(A.n_rows, dtype=np.int32)
    nb = C.c_int64()
    _lib.hcheck(lib.amgh_compact_blocks(C.byref(d), _lib.ptr(fr, C.c_uint8), max(1, (7 * int(B)) // 8), int(B), _lib.ptr(blk, C.c_int32), C.byref(nb)))
    color = np.full(A.n_rows, -1, dtype=np.int32)
    nc = C.c_int32()
    _lib.hcheck(lib.amgh_coloring_blockids(C.byref(d), _lib.ptr(fr, C.c_uint8), _lib.ptr(blk, C.c_int32), _lib.ptr(color, C.c_int32), C.byref(nc)))
    dinv = np.zeros(A.n_rows * A.br * A.br, dtype=np.float64)
    _lib.hcheck(lib.amgh_hybrid_dinv_block_ids(C.byref(d), _lib.ptr(fr, C.c_uint8), _lib.ptr(blk, C.c_int32), int(bool(pinv)), _lib.ptr(dinv, C.c_double)))
    return blk, color, int(nc.value), dinv


def _is_torch(v):
    return hasattr(v, "data_ptr") and hasattr(v, "is_cuda")


class _Vec:
    """Resolve a vector argument into (address, flags) and keep it alive for the call."""

    def __init__(self, v, n, name, writable=False):
        self.torch = _is_torch(v)
        if self.torch:
            import torch
            if not v.is_cuda:
                raise NgsAMGError(f"{name}: torch tensors must live on the GPU")
            if v.dtype != torch.float64 or not v.is_contiguous() or v.numel() != n:
                raise NgsAMGError(f"{name}: need a contiguous float64 tensor with {n} entries")
            self.obj = v
            self.addr = v.data_ptr()
        else:
            a = v if isinstance(v, np.ndarray) else np.asarray(v, dtype=np.float64)
            if a.dtype != np.float64 or not a.flags.c_contiguous or a.size != n:
                if writable:
                    raise NgsAMGError(f"{name}: need a contiguous float64 array with {n} entries")
                a = np.ascontiguousarray(a, dtype=np.float64)
                if a.size != n:
                    raise NgsAMGError(f"{name}: need {n} entries, got {a.size}")
            self.obj = a
            self.addr = a.ctypes.data


def check_multi(vecs, sizes, interleaved=False, names=None):
    """Validate the multi-vector arguments of MultMulti / MatVecMulti / SolveMulti (a plain function: no handle, no native call).

    vecs: 2-D float64, C-contiguous numpy arrays or torch CUDA tensors (all of one kind); sizes: rows each must have.
    Layout: shape (k, n) -- every right-hand side contiguous, i.e. column-major with ld = n -- or, interleaved, (n, k).
    Returns (k, addresses, leading dimensions, on_device); raises NgsAMGError for a wrong shape, dtype, stride, kind or k."""
    names = names or [f"argument {i}" for i in range(len(vecs))]
    kinds = [_is_torch(v) for v in vecs]
    if any(kinds) and not all(kinds):
        raise NgsAMGError("mixing host arrays and device tensors in one call is not supported")
    k, addrs, lds = None, [], []
    for v, n, name in zip(vecs, sizes, names):
        if _is_torch(v):
            import torch
            if not v.is_cuda:
                raise NgsAMGError(f"{name}: torch tensors must live on the GPU")
            ok_type, contig, addr = v.dtype == torch.float64, v.is_contiguous(), v.data_ptr
            shape = tuple(v.shape)
        elif isinstance(v, np.ndarray):
            ok_type, contig, addr = v.dtype == np.float64, bool(v.flags.c_contiguous), (lambda v=v: v.ctypes.data)
            shape = v.shape
        else:
            raise NgsAMGError(f"{name}: need a 2-D float64 numpy array or CUDA tensor")
        if len(shape) != 2:
            raise NgsAMGError(f"{name}: multi-vectors are 2-D, got {len(shape)} dimension(s)")
        if not ok_type:
            raise NgsAMGError(f"{name}: need float64")
        if not contig:
            raise NgsAMGError(f"{name}: need a C-contiguous array")
        kk, rows = (shape[1], shape[0]) if interleaved else shape
        if not (1 <= kk <= _lib.AMGX_MULTI_MAX):
            raise NgsAMGError(f"{name}: {kk} right-hand sides, need 1 .. {_lib.AMGX_MULTI_MAX}")
        if rows != n:
            want = f"({n}, k)" if interleaved else f"(k, {n})"
            raise NgsAMGError(f"{name}: shape {shape}, need {want}")
        if k is not None and kk != k:
            raise NgsAMGError(f"{name}: {kk} right-hand sides, the other argument has {k}")
        k = kk
        addrs.append(addr())
        lds.append(int(n))
    return k, addrs, lds, all(kinds) and bool(kinds)


def check_fuse(fuse):
    """Validate the fuse= keyword of the multi-vector calls (a plain function: no handle, no native call); returns the flag bits:
    False -> 0, True -> AMGX_MULTI_FUSE, "gs" -> AMGX_MULTI_FUSE | AMGX_MULTI_FUSE_GS (scalar Gauss-Seidel levels fuse too),
    "gs_block" -> those two | AMGX_MULTI_FUSE_GS_BLOCK (Gauss-Seidel on 2x2 / 3x3 / 6x6 levels fuses too);
    "down", "gs+down", "gs_block+down" -> the bits of True, "gs", "gs_block" | AMGX_MULTI_FUSE_DOWN (fused groups run the fused down
    pass on every level that qualifies);
    "down_dia", "gs+down_dia", "gs_block+down_dia" -> the bits of "down", "gs+down", "gs_block+down" | AMGX_MULTI_FUSE_DOWN_DIA (levels
    with a diagonal image take the fused down pass too, and such Jacobi levels the folded way up);
    "gs+f32", "gs_block+f32", "gs+down+f32", "gs_block+down+f32" -> the bits of the word before "+f32" | AMGX_MULTI_FUSE_F32 (Gauss-Seidel
    levels with single-precision images fuse too, through the multi-vector sweeps on the float arrays);
    "gs+down_f32", "gs_block+down_f32" -> the bits of "gs+down+f32", "gs_block+down+f32" | AMGX_MULTI_FUSE_DOWN_F32 (scalar Gauss-Seidel
    levels with single-precision images take the fused down pass too, the local-window form of `rest` included)"""
    if isinstance(fuse, str) and fuse in _FUSE_WORDS:
        return _FUSE_WORDS[fuse]
    if not isinstance(fuse, (bool, np.bool_)):
        raise NgsAMGError(f"fuse: need True, False, \"gs\", \"gs_block\", \"down\", \"gs+down\", \"gs_block+down\", "
                          f"\"down_dia\", \"gs+down_dia\" or \"gs_block+down_dia\", got {fuse!r}"
                          f" (or, with single-precision Gauss-Seidel images, \"gs+f32\", \"gs_block+f32\", \"gs+down+f32\", \"gs_block+down+f32\","
                          f" \"gs+down_f32\", \"gs_block+down_f32\")")
    return _lib.AMGX_MULTI_FUSE if fuse else 0


_FUSE_WORDS = {
    "gs": _lib.AMGX_MULTI_FUSE | _lib.AMGX_MULTI_FUSE_GS,
    "gs_block": _lib.AMGX_MULTI_FUSE | _lib.AMGX_MULTI_FUSE_GS | _lib.AMGX_MULTI_FUSE_GS_BLOCK,
    "down": _lib.AMGX_MULTI_FUSE | _lib.AMGX_MULTI_FUSE_DOWN,
    "gs+down": _lib.AMGX_MULTI_FUSE | _lib.AMGX_MULTI_FUSE_GS | _lib.AMGX_MULTI_FUSE_DOWN,
    "gs_block+down": _lib.AMGX_MULTI_FUSE | _lib.AMGX_MULTI_FUSE_GS | _lib.AMGX_MULTI_FUSE_GS_BLOCK | _lib.AMGX_MULTI_FUSE_DOWN,
}
# (AMGX_MULTI_FUSE_DOWN_DIA implies AMGX_MULTI_FUSE_DOWN: the words carry both bits)
_FUSE_WORDS["down_dia"] = _FUSE_WORDS["down"] | _lib.AMGX_MULTI_FUSE_DOWN_DIA
_FUSE_WORDS["gs+down_dia"] = _FUSE_WORDS["gs+down"] | _lib.AMGX_MULTI_FUSE_DOWN_DIA
_FUSE_WORDS["gs_block+down_dia"] = _FUSE_WORDS["gs_block+down"] | _lib.AMGX_MULTI_FUSE_DOWN_DIA
# (AMGX_MULTI_FUSE_F32 implies nothing: the words carry the bits of the word before "+f32" and the new one)
for _w in ("gs", "gs_block", "gs+down", "gs_block+down"):
    _FUSE_WORDS[_w + "+f32"] = _FUSE_WORDS[_w] | _lib.AMGX_MULTI_FUSE_F32
del _w
# (AMGX_MULTI_FUSE_DOWN_F32 implies AMGX_MULTI_FUSE_DOWN and AMGX_MULTI_FUSE_F32: the words carry the three bits; the Gauss-Seidel bits are the word's)
_FUSE_WORDS["gs+down_f32"] = _FUSE_WORDS["gs+down+f32"] | _lib.AMGX_MULTI_FUSE_DOWN_F32
_FUSE_WORDS["gs_block+down_f32"] = _FUSE_WORDS["gs_block+down+f32"] | _lib.AMGX_MULTI_FUSE_DOWN_F32


def hierarchy_desc(hierarchy, sm_type="gs", omega=0.9, sm_steps=1, sm_symm=False, mg_cycle="V", clev="inv", device=0,
                   use_graph=True, cheb_degree=2, cheb_ratio=10, cheb_lambda_max=None, mat_prec="double", jacobi_prec="double"):
    """amgx_hierarchy_desc over the host arrays of a hierarchy.  Returns (desc, keep): `keep` holds everything the
    descriptor points to and must outlive the amgx_create / amgx_dist_create call.
    cheb_*: levels with sm_type "cheby" (each a scalar or a per-level list); the descriptor carries 0 for a default
    (degree 2, ratio 10) and for a lambda_max that amgx_create estimates on the device.
    mat_prec: "double" (default), "single" (single-precision storage of A for the smoother passes of the Chebyshev levels),
    "single_gs" (the same, and the images of the block Gauss-Seidel sweeps), "single_gs_all" (the same, and the images of the
    scalar Gauss-Seidel sweeps) or a per-level list; see mat_prec_levels.
    jacobi_prec: "double" (default), "single" (single-precision images of A, A', Q and the diagonal image for the passes of the
    scalar Jacobi levels), "single_wide" (its A/B twin) or a per-level list; see jacobi_prec_levels."""
    levels = hierarchy.levels
    n = len(levels)
    types = sm_type if isinstance(sm_type, (list, tuple)) else [sm_type] * n
    if len(types) != n:
        raise NgsAMGError("sm_type list must have one entry per level")
    prec = mat_prec_levels(mat_prec, types)
    jprec = jacobi_prec_levels(jacobi_prec, types, [lv.A.br for lv in levels])
    arr = (_lib.amgx_level_desc * n)()
    keep = [arr, hierarchy]
    info = [None] * n            # per level: block-hybrid Gauss-Seidel data actually used (tests configure the oracle with it)
    for i, lv in enumerate(levels):
        d = arr[i]
        d.A = lv.A.desc(_lib.amgx_matrix)
        if lv.P is not None:
            d.P = lv.P.desc(_lib.amgx_matrix)
            d.PT = lv.PT.desc(_lib.amgx_matrix)
        d.dinv = _lib.ptr(lv.dinv, C.c_double)
        d.free_dofs = _lib.ptr(lv.free, C.c_uint8)
        if types[i] not in _SM:
            raise NgsAMGError(f"unknown smoother type '{types[i]}' (jacobi | gs | hgs | bgs | cheby)")
        d.sm_type = _SM[types[i]]
        if types[i] == "cheby":
            deg, lam, rat = cheby_args(cheb_degree, cheb_ratio, cheb_lambda_max, i, n)
            d.cheb_degree = deg
            d.cheb_lambda_max = lam
            d.cheb_ratio = 0.0 if rat == 10.0 else rat
        # ("single_gs" leaves a scalar Gauss-Seidel level fp64; "single_gs_all" asks for its images, 5.21, and is
        #  "single_gs" on a block level)
        if types[i] in ("gs", "hgs") and lv.A.br == 1:
            d.mat_prec = prec[i] if prec[i] == _lib.AMGX_PREC_F32_SCALAR_GS else 0
        else:
            d.mat_prec = _lib.AMGX_PREC_F32 if prec[i] == _lib.AMGX_PREC_F32_SCALAR_GS else prec[i]
        d.jacobi_prec = jprec[i]
        d.omega = float(omega)
        d.sm_steps = int(sm_steps[i] if isinstance(sm_steps, (list, tuple)) else sm_steps)      # per level: ..._spec flags
        d.sm_symm = int(bool(sm_symm[i] if isinstance(sm_symm, (list, tuple)) else sm_symm))
        d.color = _lib.ptr(lv.color, C.c_int32)
        d.n_colors = int(lv.n_colors)
        if types[i] == "hgs" and i + 1 < n:
            pre = getattr(lv, "hgs_pre", None)      # rank-partitioned levels: computed by the distributed setup (needs ghost diagonals)
            B = pre["B"] if pre else gs_block_rows(lv.A)
            if B > 0:
                import os
                pinv = bool(getattr(getattr(hierarchy, "options", None), "regularize_cmats", 0))
                blk = None
                bcolr, nbc = None, 0
                # square-block levels big enough to be bandwidth-bound: block-COLOURED sweeps (exact Gauss-Seidel between the sweep
                # blocks as well, one launch per block colour) -- PCG iterations of the sequential order (cfg 3: 16 -> 20 with the
                # hybrid form's frozen couplings between grid lines); small levels keep the single launch of the hybrid form
                bc_min = int(os.environ.get("AMGX_BGSB_BC_MIN_ROWS", "50000"))
                if pre:
                    col, nc, dinv = pre["color"], pre["n_colors"], pre["dinv"]
                elif lv.A.br > 1 and lv.A.n_rows >= bc_min and not os.environ.get("AMGX_BGSB_COMPACT") and not os.environ.get("AMGX_NO_BGSB_BC"):
                    col, nc, bcolr, nbc, dinv = block_colored_gs_data(lv.A, lv.free, B, lv.dinv)
                    # a launch per block colour must still fill the chip (256 CUs): an unstructured coarse level with 2 k sweep blocks
                    # in 9 colours (cfg 3 level 1) would run 230 workgroups per launch -- such levels keep the hybrid form
                    wg_min = int(os.environ.get("AMGX_BGSB_BC_MIN_WG", "1024")) if bc_min > 0 else 0
                    if ((lv.A.n_rows + B - 1) // B) < wg_min * max(1, nbc):
                        bcolr, nbc = None, 0
                        col, nc, dinv = hybrid_gs_data(lv.A, lv.free, B, pinv)
                elif lv.A.br > 1 and os.environ.get("AMGX_BGSB_COMPACT"):
                    # block levels: compact sweep blocks (amgh_compact_blocks) freeze half as many couplings as runs of consecutive
                    # rows (= grid lines) and bring the PCG count to within one of the sequential sweep (cfg 3: 17 vs 16; line
                    # blocks 20), but the in-block colour phases then carry half of A and run one slice per wave and phase:
                    # 250 instead of 467 applications/s at cfg 3, 128 instead of 223 at cfg 5 -- not the default
                    blk, col, nc, dinv = hybrid_gs_data_compact(lv.A, lv.free, B, pinv)
                else:
                    col, nc, dinv = hybrid_gs_data(lv.A, lv.free, B, pinv)
                info[i] = dict(B=B, color=col, n_colors=nc, dinv=dinv, block_of_row=blk, block_color=bcolr, n_block_colors=nbc)
                keep.append(info[i])
                d.color, d.n_colors, d.dinv, d.gs_block_rows = _lib.ptr(col, C.c_int32), nc, _lib.ptr(dinv, C.c_double), B
                if blk is not None:
                    d.gs_block_ids = _lib.ptr(blk, C.c_int32)
                if bcolr is not None:
                    d.gs_block_color, d.gs_n_block_colors = _lib.ptr(bcolr, C.c_int32), nbc
        g = getattr(lv, "bgs", None)
        if types[i] == "bgs" and g is None and i + 1 < n:
            raise NgsAMGError("sm_type 'bgs' needs block data on every smoothed level (Hierarchy.build_bgs())")
        if types[i] == "bgs" and g is not None:
            keep.append(g)
            d.bgs_n_blocks = int(g.n_blocks)
            d.bgs_block_ptr, d.bgs_block_rows = _lib.ptr(g.block_ptr, C.c_int32), _lib.ptr(g.block_rows, C.c_int32)
            d.bgs_dinv_ptr, d.bgs_dinv = _lib.ptr(g.dinv_ptr, C.c_int64), _lib.ptr(g.dinv, C.c_double)
            d.bgs_color, d.bgs_n_colors = _lib.ptr(g.color, C.c_int32), int(g.n_colors)
        q = getattr(lv, "Q", None)        # caller-supplied folded prolongation (rank-partitioned levels, dist.py)
        if q is not None:
            d.Q = q.desc(_lib.amgx_matrix)
    desc = _lib.amgx_hierarchy_desc()
    desc.n_levels = n
    desc.levels = arr
    if mg_cycle not in _lib.AMGX_CYCLE:
        raise NgsAMGError(f"unknown mg_cycle '{mg_cycle}' (V | W | BS)")
    desc.cycle = _lib.AMGX_CYCLE[mg_cycle]
    desc.clev = _lib.AMGX_CLEV_INV if clev == "inv" else _lib.AMGX_CLEV_NONE
    L = levels
    if clev == "inv" and hierarchy.coarse_n == 0 and n > 0 and L[-1].A.n_rows == L[-1].A.n_cols and L[-1].A.n_rows > 0:
        # the host setup hands over a dense inverse for up to 4096 unknowns; a larger coarsest level is inverted by
        # amgx_create on the device (reference: the coarsest matrix is ALWAYS inverted, amg_pc.cpp:843-928)
        desc.coarse_n = L[-1].A.n_rows * L[-1].A.br
        desc.coarse_inv = None
    else:
        desc.coarse_n = hierarchy.coarse_n if clev == "inv" else 0
        desc.coarse_inv = _lib.ptr(hierarchy.coarse_inv, C.c_double) if clev == "inv" else None
    desc.device = int(device)
    desc.use_graph = int(bool(use_graph))
    return desc, keep, info


class DeviceAMGMatrix:
    def __init__(self, hierarchy, sm_type="gs", omega=0.9, sm_steps=1, sm_symm=False, mg_cycle="V",
                 clev="inv", device=0, use_graph=True, cheb_degree=2, cheb_ratio=10, cheb_lambda_max=None, mat_prec="double",
                 jacobi_prec="double"):
        if jacobi_prec != "double":          # (the same: refused before the library is loaded)
            jacobi_prec_levels(jacobi_prec, list(sm_type) if isinstance(sm_type, (list, tuple)) else [sm_type] * len(hierarchy.levels),
                               [lv.A.br for lv in hierarchy.levels])
        if mat_prec != "double":             # a request that cannot be met is refused before the library is loaded
            n_lev = len(hierarchy.levels)
            mat_prec_levels(mat_prec, list(sm_type) if isinstance(sm_type, (list, tuple)) else [sm_type] * n_lev)
        lib = _lib.hip()
        self._lib = lib
        self._cfg = dict(sm_type=sm_type, omega=omega, sm_steps=sm_steps, sm_symm=sm_symm, mg_cycle=mg_cycle, clev=clev,
                         device=device, use_graph=use_graph, cheb_degree=cheb_degree, cheb_ratio=cheb_ratio,
                         cheb_lambda_max=cheb_lambda_max, mat_prec=mat_prec, jacobi_prec=jacobi_prec)
        self.hierarchy = hierarchy
        desc, self._keep, self.hgs = hierarchy_desc(hierarchy, sm_type, omega, sm_steps, sm_symm, mg_cycle, clev, device, use_graph,
                                                    cheb_degree, cheb_ratio, cheb_lambda_max, mat_prec, jacobi_prec)
        self._h = C.c_void_p()
        self._owned = True
        if lib.amgx_create(C.byref(desc), C.byref(self._h)) != 0:
            raise NgsAMGError(lib.amgx_last_error(None).decode())
        self._set_sizes()

    def _set_sizes(self):
        levels = self.hierarchy.levels
        self.sizes = [lv.A.n_rows * lv.A.br for lv in levels]
        self.ext_sizes = [lv.A.n_cols * lv.A.bc for lv in levels]      # > sizes on rank-partitioned levels (ghost columns)
        self.n_levels = len(levels)
        self._stream = None

    @classmethod
    def view(cls, handle, hierarchy):
        """borrowed handle (amgx_dist_handles): queries and measurement hooks of a hierarchy owned by a communicator"""
        self = cls.__new__(cls)
        self._lib = _lib.hip()
        self.hierarchy = hierarchy
        self._h = handle
        self._owned = False
        self._keep = []
        self._cfg = {}
        self.hgs = [None] * len(hierarchy.levels)
        self._set_sizes()
        return self

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and getattr(self, "_owned", True):
            self._lib.amgx_destroy(h)
        self._h = None

    # ------------------------------------------------------------------------------------------
    def _ck(self, rc):
        if rc != 0:
            raise NgsAMGError(self._lib.amgx_last_error(self._h).decode())

    def _flags(self, *vecs, graph=True):
        t = [v.torch for v in vecs]
        if any(t) and not all(t):
            raise NgsAMGError("mixing host arrays and device tensors in one call is not supported")
        f = _lib.AMGX_DEVICE_PTR if all(t) and t else _lib.AMGX_HOST_PTR
        if all(t) and t:
            import torch
            s = int(torch.cuda.current_stream().cuda_stream)
            if s != self._stream:
                self._ck(self._lib.amgx_set_stream(self._h, C.c_void_p(s)))
                self._stream = s
        if not graph:
            f |= _lib.AMGX_NO_GRAPH
        return f

    def synchronize(self):
        self._ck(self._lib.amgx_synchronize(self._h))

    def _size(self, level):
        if not (0 <= level < self.n_levels):
            raise NgsAMGError(f"level {level} out of range (0..{self.n_levels - 1})")
        return self.sizes[level]

    # AMGMatrix::Mult / MultAdd ---------------------------------------------------------------
    def Mult(self, b, x, graph=True):
        vb, vx = _Vec(b, self.sizes[0], "b"), _Vec(x, self.sizes[0], "x", True)
        self._ck(self._lib.amgx_apply(self._h, vb.addr, vx.addr, 0, self._flags(vb, vx, graph=graph)))
        return x

    def MultAdd(self, s, b, x, graph=True):
        vb, vx = _Vec(b, self.sizes[0], "b"), _Vec(x, self.sizes[0], "x", True)
        self._ck(self._lib.amgx_apply_add(self._h, float(s), vb.addr, vx.addr, self._flags(vb, vx, graph=graph)))
        return x

    MultTrans = Mult
    MultTransAdd = MultAdd

    # multi-vectors: BaseMatrix::Mult on a MultiVector, k right-hand sides per matrix pass (amgx_apply_multi) ----------
    def _multi_flags(self, on_device, interleaved, graph=True):
        f = _lib.AMGX_DEVICE_PTR if on_device else _lib.AMGX_HOST_PTR
        if on_device:
            import torch
            s = int(torch.cuda.current_stream().cuda_stream)
            if s != self._stream:
                self._ck(self._lib.amgx_set_stream(self._h, C.c_void_p(s)))
                self._stream = s
        if interleaved:
            f |= _lib.AMGX_MULTI_INTERLEAVED
        if not graph:
            f |= _lib.AMGX_NO_GRAPH
        return f

    def MultMulti(self, B, X, interleaved=False, graph=True, fuse=False):
        """X[j] = C B[j] for k = 1 .. 8 right-hand sides: 2-D float64 arrays / CUDA tensors of shape (k, n), or (n, k) with
        interleaved=True.  Handles that qualify (multi_info) read every level matrix once per group of 2, 4 or 8 columns.
        fuse=True (AMGX_MULTI_FUSE): the wider rule of multi_plan(k, fuse=True) -- Chebyshev and block levels run fused too.
        fuse="gs" (AMGX_MULTI_FUSE_GS as well): scalar Gauss-Seidel levels (block-hybrid or multicolour form) run fused too.
        fuse="gs_block" (AMGX_MULTI_FUSE_GS_BLOCK as well): so does Gauss-Seidel on 2x2 / 3x3 / 6x6 levels (hybrid-block,
        block-coloured and multicolour forms) -- the default smoother of the elasticity hierarchies.
        fuse="down", "gs+down", "gs_block+down" (AMGX_MULTI_FUSE_DOWN beside the bits of True, "gs", "gs_block"): the fused groups
        run the residual + restriction of every level that qualifies in one pass (multi_level_plan).
        fuse="down_dia", "gs+down_dia", "gs_block+down_dia" (AMGX_MULTI_FUSE_DOWN_DIA as well): levels with a diagonal image qualify
        too, and a Jacobi level that takes the pass runs the way up as x = z + Q x_c.
        fuse="gs+f32", "gs_block+f32", "gs+down+f32", "gs_block+down+f32" (AMGX_MULTI_FUSE_F32 as well): Gauss-Seidel levels with
        single-precision images (mat_prec="single_gs_all" / "single_gs") run fused too, on the float arrays.
        fuse="gs+down_f32", "gs_block+down_f32" (AMGX_MULTI_FUSE_DOWN_F32 as well): the scalar levels of such a handle take the fused
        down pass on their float `rest` image too (sell, sell-win and the local-window form "sell-lw": multi_level_plan)."""
        ff = check_fuse(fuse)
        n = self.sizes[0]
        k, (ab, ax), (lb, lx), dev = check_multi((B, X), (n, n), interleaved, ("B", "X"))
        self._ck(self._lib.amgx_apply_multi(self._h, k, ab, lb, ax, lx, 0, self._multi_flags(dev, interleaved, graph) | ff))
        return X

    def MatVecMulti(self, level, X, Y, interleaved=False, fuse=False):
        """Y[j] = A_level X[j]"""
        ff = check_fuse(fuse)
        n = self._size(level)
        k, (ax, ay), (lx, ly), dev = check_multi((X, Y), (self.ext_sizes[level], n), interleaved, ("X", "Y"))
        self._ck(self._lib.amgx_matvec_multi(self._h, int(level), k, ax, lx, ay, ly, self._multi_flags(dev, interleaved) | ff))
        return Y

    def multi_plan(self, k, fuse=False):
        """multi_info for a call that carries fuse=, plus "note": the first reason why the handle is not fused ("" when it is).
        A handle with single-precision Gauss-Seidel images answers fused under "gs+f32" / "gs_block+f32" only."""
        ff = check_fuse(fuse)
        if not (1 <= int(k) <= _lib.AMGX_MULTI_MAX):
            raise NgsAMGError(f"multi_plan: k = {k}, need 1 .. {_lib.AMGX_MULTI_MAX}")
        fused, ng, wb = C.c_int32(), C.c_int32(), C.c_int64()
        wd = (C.c_int32 * _lib.AMGX_MULTI_MAX)()
        self._ck(self._lib.amgx_multi_plan(self._h, int(k), ff, C.byref(fused), C.byref(ng), wd, C.byref(wb)))
        note = self._lib.amgx_multi_note(self._h, ff) or b""
        return {"fused": int(fused.value), "groups": [int(wd[i]) for i in range(ng.value)], "work_bytes": int(wb.value),
                "note": note.decode()}

    _LEVEL_PLAN_FORMS = ("literal", "sell", "sell-win", "dia", "dia-box")
    _LEVEL_PLAN_FORMS_ALL = _LEVEL_PLAN_FORMS + ("sell-lw",)                 # form 5: under AMGX_MULTI_FUSE_DOWN_F32 alone

    def multi_level_plan(self, level, fuse=False):
        """the down pass of one level in a fused group of a call that carries fuse= (amgx_multi_level_plan): "form" ("literal", "sell",
        "sell-win", with a "..._dia" word "dia" / "dia-box", with a "...+down_f32" word on a level with single-precision Gauss-Seidel
        images "sell-lw"), "mode" (0 Jacobi from zero, 1 after a block-hybrid sweep, 2 after Chebyshev), "folded_up", "float_image" (the launch
        reads a float array), "lds_bytes" (per workgroup on 4 vectors) and "note", the reason a level stays literal ("" when it does not);
        "lanes", "ept" and "lw_max_list": lanes per row, entries of P per thread and the longest column list of a local-window chunk of
        the level's fused down plan, whether or not a fused group takes it (0 without a plan or without a "down" word)"""
        ff = check_fuse(fuse)
        if isinstance(level, bool) or not isinstance(level, (int, np.integer)):
            raise NgsAMGError(f"multi_level_plan: level must be an integer, got {level!r}")
        self._size(int(level))
        out = (C.c_int32 * 8)()
        self._ck(self._lib.amgx_multi_level_plan(self._h, int(level), ff, out, 8))
        note = self._lib.amgx_multi_level_note(self._h, int(level), ff) or b""
        return {"form": self._LEVEL_PLAN_FORMS_ALL[int(out[0])],"mode": int(out[1]), "folded_up": bool(out[2]), "float_image": bool(out[3]),
                "lds_bytes": int(out[4]), "out": [int(v) for v in out[:5]], "note": note.decode(),
                "lanes": int(out[5]), "ept": int(out[6]), "lw_max_list": int(out[7])}

    def DownMulti(self, level, B, X=None, x_given=False, interleaved=False, fuse=False):
        """the down stage of a level per column (amgx_down_multi); returns (X, BC).  B: (k, n_level), or (n_level, k) with
        interleaved=True.  x_given=False: X is output (allocated like B when None): pre-smoothing from zero, then BC[j] = P^T (B[j] -
        A X[j]) -- the down stage of the V-cycle, X holds z on a level with the folded prolongation.  x_given=True: X is the
        iterate after the level's pre-smoothing and only the residual + restriction half runs.  fuse="down" / "gs+down": groups of 4
        and 2 columns run the multi-vector kernels where the level qualifies (multi_level_plan); a column is the same bit for
        bit either way.  fuse="gs+down_f32": so do the scalar Gauss-Seidel levels of a handle with single-precision images, on the
        float array the single-vector launch reads."""
        ff = check_fuse(fuse)
        if not isinstance(x_given, (bool, np.bool_)):
            raise NgsAMGError(f"DownMulti: x_given must be True or False, got {x_given!r}")
        if isinstance(level, bool) or not isinstance(level, (int, np.integer)):
            raise NgsAMGError(f"DownMulti: level must be an integer, got {level!r}")
        level = int(level)
        n = self._size(level)
        if level + 1 >= self.n_levels:
            raise NgsAMGError(f"DownMulti: level {level} is the coarsest level (no restriction)")
        if self.ext_sizes[level] != n:
            raise NgsAMGError(f"DownMulti: level {level} carries ghost columns (rank-partitioned levels are not supported)")
        if X is None:
            if x_given:
                raise NgsAMGError("DownMulti: x_given=True needs X")
            if _is_torch(B):
                import torch
                X = torch.empty_like(B)
            elif isinstance(B, np.ndarray):
                X = np.empty_like(B)
            else:
                raise NgsAMGError("B: need a 2-D float64 numpy array or CUDA tensor")
        k, (ab, ax), (lb, lx), dev = check_multi((B, X), (n, n), interleaved, ("B", "X"))
        nc = self.sizes[level + 1]
        shape = (nc, k) if interleaved else (k, nc)
        if dev:
            import torch
            BC = torch.empty(shape, dtype=torch.float64, device=B.device)
            ac = BC.data_ptr()
        else:
            BC = np.empty(shape)
            ac = BC.ctypes.data
        self._ck(self._lib.amgx_down_multi(self._h, level, k, ab, lb, ax, lx, ac, nc, int(bool(x_given)),
                                           self._multi_flags(dev, interleaved) | ff))
        return X, BC

    def multi_info(self, k):
        """how a multi-vector call with k columns runs: fused (True: the multi-vector kernels; False: a column loop over the
        single-vector path), the widths of the column groups and the bytes of multi-vector work space"""
        if not (1 <= int(k) <= _lib.AMGX_MULTI_MAX):
            raise NgsAMGError(f"multi_info: k = {k}, need 1 .. {_lib.AMGX_MULTI_MAX}")
        fused, ng, wb = C.c_int32(), C.c_int32(), C.c_int64()
        wd = (C.c_int32 * _lib.AMGX_MULTI_MAX)()
        self._ck(self._lib.amgx_multi_info(self._h, int(k), C.byref(fused), C.byref(ng), wd, C.byref(wb)))
        return {"fused": int(fused.value), "groups": [int(wd[i]) for i in range(ng.value)], "work_bytes": int(wb.value)}

    def apply(self, b):
        """convenience: returns a new vector C b of the same kind as b"""
        if _is_torch(b):
            import torch
            x = torch.empty_like(b)
        else:
            x = np.empty(self.sizes[0])
        return self.Mult(b, x)

    def SmoothMulti(self, level, X, B, x_zero=False, back=False, interleaved=False, fuse=False):
        """one plain smoother step per column: Smooth(level, X[j], B[j], res, x_zero=x_zero, back=back) with a res of its own
        (amgx_smooth_multi).  X, B: (k, n_level), or (n_level, k) with interleaved=True.  fuse="gs": groups of 4 and 2 columns
        run the multi-vector Gauss-Seidel sweeps on a scalar level that has them, fuse="gs_block" on a square-block level too;
        fuse="gs+f32" / "gs_block+f32" also on a level whose sweeps read single-precision images (the float sweeps).  A column
        equals Smooth bit for bit either way."""
        ff = check_fuse(fuse)
        n = self._size(level)
        if self.ext_sizes[level] != n:
            raise NgsAMGError(f"SmoothMulti: level {level} carries ghost columns (rank-partitioned levels are not supported)")
        k, (ax, ab), (lx, lb), dev = check_multi((X, B), (n, n), interleaved, ("X", "B"))
        self._ck(self._lib.amgx_smooth_multi(self._h, int(level), 1 if back else 0, k, ax, lx, ab, lb, int(bool(x_zero)),
                                             self._multi_flags(dev, interleaved) | ff))
        return X

    # smoothers ---------------------------------------------------------------------------------
    def Smooth(self, level, x, b, res, res_updated=False, update_res=False, x_zero=False, back=False):
        n = self._size(level)
        vx, vb, vr = _Vec(x, self.ext_sizes[level], "x", True), _Vec(b, n, "b"), _Vec(res, n, "res", True)
        self._ck(self._lib.amgx_smooth(self._h, level, 1 if back else 0, vx.addr, vb.addr, vr.addr,
                                       int(res_updated), int(update_res), int(x_zero), self._flags(vx, vb, vr)))

    def SmoothVFromLevel(self, level, x, b, res, res_updated=False, update_res=False, x_zero=False):
        n = self._size(level)
        vx, vb, vr = _Vec(x, n, "x", True), _Vec(b, n, "b"), _Vec(res, n, "res", True)
        self._ck(self._lib.amgx_smooth_v_from_level(self._h, level, vx.addr, vb.addr, vr.addr, int(res_updated),
                                                    int(update_res), int(x_zero), self._flags(vx, vb, vr)))

    # stage entry points for rank-partitioned levels (ghost entries of the gathered vector filled by the caller) ----
    def JacobiPre(self, level, b_ext, x, r):
        vb, vx, vr = _Vec(b_ext, self.ext_sizes[level], "b"), _Vec(x, self._size(level), "x", True), _Vec(r, self._size(level), "r", True)
        self._ck(self._lib.amgx_jacobi_pre(self._h, level, vb.addr, vx.addr, vr.addr, self._flags(vb, vx, vr)))

    def CycleDown(self, level, b_ext, x, b_coarse):
        """x = two Jacobi steps from zero on b (no coarse correction yet), b_coarse = P^T (b - A w Dinv b)"""
        vb, vx = _Vec(b_ext, self.ext_sizes[level], "b"), _Vec(x, self._size(level), "x", True)
        vc = _Vec(b_coarse, self._size(level + 1), "b_coarse", True)
        self._ck(self._lib.amgx_cycle_down(self._h, level, vb.addr, vx.addr, vc.addr, self._flags(vb, vx, vc)))

    def CycleUp(self, level, x, x_coarse_ext):
        """x += Q x_coarse: coarse-grid correction and Jacobi post-smoothing in one product"""
        vx, vc = _Vec(x, self._size(level), "x", True), _Vec(x_coarse_ext, self.q_cols(level), "x_coarse")
        self._ck(self._lib.amgx_cycle_up(self._h, level, vx.addr, vc.addr, self._flags(vx, vc)))

    def is_folded(self, level):
        return self.matrix_info(level, "Q")["fmt"] is not None

    def q_cols(self, level):
        q = getattr(self.hierarchy.levels[level], "Q", None)
        return q.n_cols if q is not None else self.hierarchy.levels[level].P.n_cols

    def JacobiPost(self, level, x_in_ext, b, x_out):
        vi, vb, vo = _Vec(x_in_ext, self.ext_sizes[level], "x_in"), _Vec(b, self._size(level), "b"), _Vec(x_out, self._size(level), "x_out", True)
        self._ck(self._lib.amgx_jacobi_post(self._h, level, vi.addr, vb.addr, vo.addr, self._flags(vi, vb, vo)))

    def Residual(self, level, x_ext, b, r):
        vx, vb, vr = _Vec(x_ext, self.ext_sizes[level], "x"), _Vec(b, self._size(level), "b"), _Vec(r, self._size(level), "r", True)
        self._ck(self._lib.amgx_residual(self._h, level, vx.addr, vb.addr, vr.addr, self._flags(vx, vb, vr)))

    def Prolong(self, level, fac, x_in, x_coarse, x_out):
        nc = self.hierarchy.levels[level].P.n_cols * self.hierarchy.levels[level].P.bc
        vi, vc, vo = _Vec(x_in, self._size(level), "x_in"), _Vec(x_coarse, nc, "x_coarse"), _Vec(x_out, self._size(level), "x_out", True)
        self._ck(self._lib.amgx_prolong(self._h, level, float(fac), vi.addr, vc.addr, vo.addr, self._flags(vi, vc, vo)))

    # matrices / transfers ---------------------------------------------------------------------
    def MatVec(self, level, x, y):
        n = self._size(level)
        vx, vy = _Vec(x, self.ext_sizes[level], "x"), _Vec(y, n, "y", True)
        self._ck(self._lib.amgx_matvec(self._h, level, vx.addr, vy.addr, self._flags(vx, vy)))
        return y

    def TransferF2C(self, level, x_fine, x_coarse):
        vf, vc = _Vec(x_fine, self._size(level), "x_fine"), _Vec(x_coarse, self._size(level + 1), "x_coarse", True)
        self._ck(self._lib.amgx_transfer_f2c(self._h, level, vf.addr, vc.addr, self._flags(vf, vc)))
        return x_coarse

    def AddC2F(self, level, fac, x_fine, x_coarse):
        vf, vc = _Vec(x_fine, self._size(level), "x_fine", True), _Vec(x_coarse, self._size(level + 1), "x_coarse")
        self._ck(self._lib.amgx_add_c2f(self._h, level, float(fac), vf.addr, vc.addr, self._flags(vf, vc)))
        return x_fine

    def CoarseSolve(self, rhs, x):
        n = self.sizes[-1]
        vr, vx = _Vec(rhs, n, "rhs"), _Vec(x, n, "x", True)
        self._ck(self._lib.amgx_coarse_solve(self._h, vr.addr, vx.addr, self._flags(vr, vx)))
        return x

    # queries ------------------------------------------------------------------------------------
    def GetNLevels(self, rank=0):
        return self._lib.amgx_n_levels(self._h)

    def level_info(self, level):
        n, bs, nnz = C.c_int64(), C.c_int32(), C.c_int64()
        self._ck(self._lib.amgx_level_info(self._h, level, C.byref(n), C.byref(bs), C.byref(nnz)))
        return n.value, bs.value, nnz.value

    def cycle_info(self):
        """how the V-cycle is launched: first level of the single-workgroup tail kernel, first level of the collapsed
        (dense) coarse levels and the size of that dense operator (-1 / 0: not used)"""
        t, d, n = C.c_int32(), C.c_int32(), C.c_int64()
        self._ck(self._lib.amgx_cycle_info(self._h, C.byref(t), C.byref(d), C.byref(n)))
        return {"tail_level": t.value, "dense_level": d.value, "dense_n": n.value}

    _WHICH = {"A": 0, "P": 1, "PT": 2, "Apre": 3, "Q": 4, "ApreLW": 5, "QLW": 6, "A32": 7}

    def matrix_info(self, level, which):
        """device format of one image of a level ("A32": the single-precision image of A that the smoother passes read, fmt None
        where the level has none)"""
        fmt, stored, lanes = C.c_int32(), C.c_int64(), C.c_int32()
        self._ck(self._lib.amgx_matrix_info(self._h, level, self._WHICH[which], C.byref(fmt), C.byref(stored), C.byref(lanes)))
        nb = C.c_int64()
        self._ck(self._lib.amgx_matrix_stream_bytes(self._h, level, self._WHICH[which], C.byref(nb)))
        return {"fmt": {-1: None, 0: "csrvec", 1: "sell", 2: "bsell", 3: "sellwin", 4: "rigid-body", 5: "sell-lw", 6: "dia"}.get(fmt.value, "?"), "stored": stored.value, "lanes": lanes.value,
                "stream_bytes": nb.value}

    _PATH_KEYS = ("kernel", "fused_block", "lanes", "ept", "compact", "max_slots", "max_entries", "dia_k", "xcd_A", "xcd_Apre",
                  "xcd_Q", "xcd_dia", "A_slices16", "A_slices", "Apre_slices16", "Apre_slices", "lw_no_window", "folded", "chunks",
                  "gs_form", "gs_lanes", "gs_threads", "gs_block", "gs_colors", "gs_block_colors", "gs_split", "gs_lowin_maxw",
                  "gs_full_maxw", "gs_narrow", "gs_mid", "gs_lw", "gs_w_mask", "gs_lw_no_window", "gs_down",
                  "bgs_threads", "bgs_lanes", "bgs_max_m", "bcsr_A", "bcsr_P", "bcsr_PT")
    _GS_FORMS = {0: None, 1: "mc", 2: "mc-block-rowlist", 3: "mc-block-bsell", 4: "hybrid", 5: "hybrid-block", 6: "block-coloured",
                 7: "bgs"}

    def level_paths(self, level):
        """the paths amgx_create chose for one level (amgx_level_paths, read-only): the fused Jacobi down kernel (None, "sell",
        "sell-win", "sell-lw" or "dia"), its workgroup size and lanes per row, the chunk-local restriction (entries of P per thread,
        "compact": 0 consecutive rows / 1 compact chunks / 2 box chunks of the DIA image, most slots / entries in one chunk, number
        of chunks), the diagonals of the DIA image, the XCD placement
        flags, the 16-bit / all slices of A and A', the local-window chunks without a window and whether the level is folded;
        the Gauss-Seidel sweep ("gs_form": None, "mc", "mc-block-rowlist", "mc-block-bsell", "hybrid", "hybrid-block",
        "block-coloured" or "bgs"), its lanes per row, workgroup size, rows per block, colours, block colours, split images, the
        widest slices of the block-hybrid images, the block-hybrid kernel choices (narrow sweep from zero, mid-width and
        local-window general sweep, blocks of the local-window image without a window), the row-list kernel's lanes per block
        row (bitmask of W) and the form of the block-hybrid down pass's fused residual + restriction ("gs_down": None, "sell",
        "sell-win" or "sell-lw"); the aggregate block Gauss-Seidel kernel ("bgs_threads", "bgs_lanes": TH and G of
        bgs_block_kernel<BS, TH, G>, "bgs_max_m": scalar dofs of the largest block) and the kernel of a product with A, P, P^T in
        the block CSR format ("bcsr_A", "bcsr_P", "bcsr_PT": None, ("rowlane", W) or ("csrvec", G))"""
        out = np.zeros(len(self._PATH_KEYS), dtype=np.int64)
        self._ck(self._lib.amgx_level_paths(self._h, int(level), out.ctypes.data_as(_lib.c_i64p), out.size))
        d = dict(zip(self._PATH_KEYS, (int(v) for v in out)))
        d["kernel"] = {0: None, 1: "sell", 2: "sell-win", 3: "sell-lw", 4: "dia", 5: "cheby-res"}[d["kernel"]]
        d["gs_form"] = self._GS_FORMS[d["gs_form"]]
        d["gs_down"] = {0: None, 1: "sell", 2: "sell-win", 3: "sell-lw"}[d["gs_down"]]
        for k in ("bcsr_A", "bcsr_P", "bcsr_PT"):
            d[k] = None if d[k] == 0 else (("rowlane", "csrvec")[d[k] // 100 - 1], d[k] % 100)
        return d

    _EXTRA_KEYS = ("tail_ops", "tail_gs_lds", "gs_slices16", "gs_slices", "gs_rowrel", "A_diag_first", "Apre_diag_first", "Apre_wdiag",
                   "graphs", "gs_f32", "gs_f32_images", "gs_f32_bytes")

    def level_extra(self, level):
        """further read-only paths of one level (amgx_level_extra): the operations of the tail kernel's program ("tail_ops", 0
        without such a tail), the form of this level's Gauss-Seidel sweeps inside it ("tail_gs_lds": 1 x in LDS, 0 x in global
        memory, None not a Gauss-Seidel level of the tail), the 16-bit / all slices of the colour-major copies of the multicolour
        scalar sweep and whether their 16-bit columns are row-relative, whether the sliced-ELL images of A and A' store the diagonal
        entry of every row first and whether that slot of A' holds omega, the whole-cycle graphs the handle holds, and the
        single-precision images of a Gauss-Seidel block level (mat_prec "single_gs"): whether the sweeps read them ("gs_f32"), how
        many there are (A included) and the bytes of their values"""
        out = np.zeros(len(self._EXTRA_KEYS), dtype=np.int64)
        self._ck(self._lib.amgx_level_extra(self._h, int(level), out.ctypes.data_as(_lib.c_i64p), out.size))
        d = dict(zip(self._EXTRA_KEYS, (int(v) for v in out)))
        d["tail_gs_lds"] = None if d["tail_gs_lds"] < 0 else d["tail_gs_lds"]
        return d

    _JPREC_KEYS = ("f32", "images", "bytes", "released", "wide")
    _JPREC_IMAGES = ("A", "Apre", "ApreLW", "dia", "Q", "QLW")

    def jacobi_prec_info(self, level):
        """what jacobi_prec gave a level (amgx_jacobi_prec_info): whether its passes read float images ("f32"; 0
        under "single_wide"), the tuple of the images converted ("images": of A, Apre, ApreLW, dia, Q, QLW; "mask": the bits), the
        value bytes of the converted arrays, the fp64 value bytes released, and whether the level is the twin ("wide")"""
        out = np.zeros(_lib.AMGX_JACOBI_PREC_INFO_N, dtype=np.int64)
        self._ck(self._lib.amgx_jacobi_prec_info(self._h, int(level), out.ctypes.data_as(_lib.c_i64p), out.size))
        d = dict(zip(self._JPREC_KEYS, (int(v) for v in out)))
        d["mask"] = d["images"]
        d["images"] = tuple(n for b, n in enumerate(self._JPREC_IMAGES) if d["mask"] >> b & 1)
        return d

    _GSPREC_IMAGES = ("A", "full", "fullLW", "lowin", "rest", "restLW", "sell", "lower", "upper")

    def gs_prec_info(self, level):
        """what mat_prec "single_gs_all" gave a scalar Gauss-Seidel level (amgx_gs_prec_info): whether its sweeps read
        float images ("f32"; 0 under AMGX_GS_F32_WIDE), the tuple of the images converted ("images": of A, full, fullLW, lowin, rest,
        restLW, sell, lower, upper; "mask": the bits), the value bytes of the converted arrays, the fp64 value bytes released, and
        whether the level is the twin ("wide")"""
        out = np.zeros(_lib.AMGX_GS_PREC_INFO_N, dtype=np.int64)
        self._ck(self._lib.amgx_gs_prec_info(self._h, int(level), out.ctypes.data_as(_lib.c_i64p), out.size))
        d = dict(zip(self._JPREC_KEYS, (int(v) for v in out)))
        d["mask"] = d["images"]
        d["images"] = tuple(n for b, n in enumerate(self._GSPREC_IMAGES) if d["mask"] >> b & 1)
        return d

    _SM_NAMES = {_lib.AMGX_SM_JACOBI: "jacobi", _lib.AMGX_SM_GS: "gs", _lib.AMGX_SM_BGS: "bgs", _lib.AMGX_SM_CHEBY: "cheby"}

    def smoother_info(self, level):
        """the smoother of a level (amgx_smoother_info): type and, for "cheby", degree, interval [lambda_min, lambda_max] of Dinv A
        and whether lambda_max was estimated on the device"""
        t, deg, est = C.c_int32(), C.c_int32(), C.c_int32()
        lmax, lmin = C.c_double(), C.c_double()
        self._ck(self._lib.amgx_smoother_info(self._h, int(level), C.byref(t), C.byref(deg), C.byref(lmax), C.byref(lmin), C.byref(est)))
        return {"sm_type": self._SM_NAMES.get(t.value, "?"), "degree": deg.value, "lambda_max": lmax.value, "lambda_min": lmin.value,
                "estimated": est.value}

    def time_op(self, level, op, reps=20):
        ms = C.c_double()
        self._ck(self._lib.amgx_time_op(self._h, level, int(op), int(reps), C.byref(ms)))
        return ms.value


# ---------------------------------------------------------------------------------------------
# byte model of SURVEY.md section 8d / BASELINE.md (algorithmic bytes per cycle)
# ---------------------------------------------------------------------------------------------

def _fetch_result(lib, res, n_rows, n_cols, nnz, br=1, bc=1):
    rp = np.zeros(n_rows + 1, dtype=np.int64)
    col = np.zeros(max(1, nnz), dtype=np.int32)
    val = np.zeros(max(1, nnz) * br * bc)
    if lib.amgx_csr_result_fetch(res, _lib.ptr(rp, C.c_int64), _lib.ptr(col, C.c_int32), _lib.ptr(val, C.c_double)) != 0:
        raise NgsAMGError(lib.amgx_last_error(None).decode())
    return Matrix(n_rows, n_cols, br, bc, rp, col[:nnz], val[:nnz * br * bc])


def device_spmm(A, B):
    """C = A B on the device (amgx_spgemm; (block-)CSR, bit-identical to the host library's amgh_matmul).
    None: the device library does not take this product (result blocks beyond 6 x 6, a row with more than 8192 products)."""
    lib = _lib.hip()
    da, db = A.desc(_lib.amgx_matrix), B.desc(_lib.amgx_matrix)
    res, nr, nnz = C.c_void_p(), C.c_int64(), C.c_int64()
    rc = lib.amgx_spgemm(C.byref(da), C.byref(db), C.byref(res), C.byref(nr), C.byref(nnz))
    if rc == 2:
        return None
    if rc != 0:
        raise NgsAMGError(lib.amgx_last_error(None).decode())
    return _fetch_result(lib, res, int(nr.value), B.n_cols, int(nnz.value), A.br, B.bc)


def device_galerkin(PT, A, P):
    """A_c = (P^T A) P on the device (amgx_galerkin); None as device_spmm."""
    lib = _lib.hip()
    dt, da, dp = PT.desc(_lib.amgx_matrix), A.desc(_lib.amgx_matrix), P.desc(_lib.amgx_matrix)
    res, nr, nnz = C.c_void_p(), C.c_int64(), C.c_int64()
    rc = lib.amgx_galerkin(C.byref(dt), C.byref(da), C.byref(dp), C.byref(res), C.byref(nr), C.byref(nnz))
    if rc == 2:
        return None
    if rc != 0:
        raise NgsAMGError(lib.amgx_last_error(None).decode())
    return _fetch_result(lib, res, int(nr.value), P.n_cols, int(nnz.value), PT.br, P.bc)


def matrix_bytes(M):
    """B(M) = nnz*(8*br*bc + 4) + 4*(n+1): fp64 values, int32 columns, int32 row pointers."""
    if M is None:
        return 0
    return M.nnz * (8 * M.br * M.bc + 4) + 4 * (M.n_rows + 1)


def vcycle_bytes(hierarchy):
    """Algorithmic bytes of one Jacobi V(1,1) cycle:
    per level 2 B(A) + B(P) + B(PT) + 16 b^2 n + 15 V_l + 2 V_{l+1}; coarsest 8 (n b)^2 + 2 V."""
    total = 0
    per_level = []
    L = hierarchy.levels
    for i, lv in enumerate(L):
        V = 8 * lv.bs * lv.n
        if i + 1 < len(L):
            Vc = 8 * L[i + 1].bs * L[i + 1].n
            b = 2 * matrix_bytes(lv.A) + matrix_bytes(lv.P) + matrix_bytes(lv.PT) + 16 * lv.bs * lv.bs * lv.n + 15 * V + 2 * Vc
        else:
            b = 8 * (lv.n * lv.bs) ** 2 + 2 * V
        per_level.append(b)
        total += b
    return total, per_level
