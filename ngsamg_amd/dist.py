"""Rank-partitioned V-cycle: one process per GPU, halo exchange between neighbours.

What the reference does with MPI (`HybridMatrix` M/G split + `DCCMap` DISTRIBUTED/CONCENTRATED/CUMULATED exchanges,
reference src/base/linalg/hybrid_matrix.cpp:17-453, dcc_map.cpp:76-302, and Jacobi "in parallel" as defined in
SURVEY.md 8e) is realised here in the row-partitioned form that maps onto the single-GPU kernels unchanged:

  * every vertex of every distributed level has exactly ONE owner rank (box partition of the structured grid on level
    0, inherited through the aggregates below); a rank stores the rows of its owned vertices, with columns
    [owned | ghost]; ghosts are sorted by (owner, owner-local index), so a neighbour's data lands contiguously;
  * aggregates never cross a rank boundary and a prolongation row only references coarse vertices of its own rank,
    hence restriction and prolongation need no communication; the Galerkin product needs the P rows of the ghost
    vertices once, at setup;
  * per cycle and distributed level there are two halo exchanges (before the two passes over A: `b` for the fused
    pre-smoothing pass, `x + P x_c` -- or the coarse solution, in the folded form -- for the way up).  The DATA PATH is
    native (csrc/device/dist.hpp behind the C ABI: amgx_comm_* / amgx_dist_apply): hand-written pack kernels, ncclSend /
    ncclRecv on a communication stream straight into the ghost segment, interior rows processed meanwhile, the whole
    cycle replayed from one hipGraph.  torch.distributed (gloo) only carries the rendezvous, the 128-byte RCCL id and
    the host messages of THIS setup; the stage-by-stage driver at the end of this file (index_select + all_gather through
    a backend object) is the CPU test backend and refuses to run where a GPU is present;
  * once a level is small it is gathered and the remaining hierarchy is REPLICATED on every rank (one all-gather of
    the level's right-hand side per cycle) - the GPU analogue of the reference's contraction to one rank
    (`CtrMap`, src/base/coarsening/dof_contract.cpp:49-223) without the extra latency hop back.

The result equals a serial Jacobi V-cycle on the global hierarchy (block-diagonal P per rank + replicated tail), which
is what the tests check against the CPU oracle.

Communication is abstracted so that the same code runs (a) one rank per process over torch.distributed and (b) several
"virtual ranks" inside one process (LoopbackComm), which is how the device path is exercised on a single GPU.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import scipy.sparse as sp

from . import _lib
from ._lib import Matrix, NgsAMGError
from .hierarchy import Hierarchy, Level


# ------------------------------------------------------------------------------------------------------------
# communication
# ------------------------------------------------------------------------------------------------------------

class LoopbackComm:
    """All `size` ranks live in this process (bulk-synchronous emulation)."""

    def __init__(self, size):
        self.size = size
        self.local_ranks = list(range(size))

    def exchange(self, sends):
        """sends[i]: dict peer -> np.ndarray for local rank i; returns recvs[i]: dict peer -> np.ndarray"""
        recvs = [dict() for _ in self.local_ranks]
        for i, d in enumerate(sends):
            for peer, arr in d.items():
                recvs[peer][i] = np.array(arr, copy=True)
        return recvs

    def allgather(self, items):
        return [list(items) for _ in self.local_ranks]

    def halo(self, bufs_send, bufs_recv):
        """device / tensor halo exchange: bufs_send[i][peer] -> bufs_recv[peer][i] (tensors, same sizes)"""
        for i, d in enumerate(bufs_send):
            for peer, t in d.items():
                bufs_recv[peer][i].copy_(t)

    def allgather_tensor(self, parts, outs, counts):
        """outs[i] = concatenation of parts[0..size) (each part has counts[r] entries)"""
        for out in outs:
            off = 0
            for r, p in enumerate(parts):
                out[off:off + counts[r]].copy_(p[:counts[r]])
                off += counts[r]

    def barrier(self):
        pass


def compaction_index(counts, m):
    """positions of the valid entries in an all-gather of pieces padded to length m (piece r holds counts[r] entries)"""
    return np.concatenate([r * m + np.arange(c) for r, c in enumerate(counts)]).astype(np.int64)


class TorchComm:
    """One rank per process; host payloads travel over a gloo group, device halos over the default (nccl) group."""

    def __init__(self, device_group=None, host_group=None):
        import torch.distributed as dist
        self.dist = dist
        self.size = dist.get_world_size()
        self.rank = dist.get_rank()
        self.local_ranks = [self.rank]
        self.device_group = device_group
        self.host_group = host_group if host_group is not None else (
            dist.new_group(backend="gloo") if dist.get_backend() != "gloo" else None)

    def exchange(self, sends):
        import torch
        dist = self.dist
        d = sends[0]
        peers = sorted(d.keys())
        # sizes first (every exchange in this module is symmetric: if I send to q, q sends to me)
        reqs, sizes = [], {}
        for q in peers:
            t = torch.tensor([d[q].size, 0], dtype=torch.int64)
            r = torch.zeros(2, dtype=torch.int64)
            sizes[q] = r
            reqs.append(dist.isend(t, q, group=self.host_group))
            reqs.append(dist.irecv(r, q, group=self.host_group))
        for r in reqs:
            r.wait()
        out, reqs, keep = {}, [], []
        for q in peers:
            n = int(sizes[q][0])
            recv = np.empty(n, dtype=d[q].dtype)          # every exchange here is symmetric in dtype
            out[q] = recv
            st = torch.from_numpy(np.ascontiguousarray(d[q]).view(np.uint8).reshape(-1).copy())
            rt = torch.from_numpy(recv.view(np.uint8).reshape(-1))
            keep += [st, rt]
            if st.numel():
                reqs.append(dist.isend(st, q, group=self.host_group))
            if rt.numel():
                reqs.append(dist.irecv(rt, q, group=self.host_group))
        for r in reqs:
            r.wait()
        return [out]

    def allgather(self, items):
        out = [None] * self.size
        self.dist.all_gather_object(out, items[0], group=self.host_group)
        return [out]

    def halo(self, bufs_send, bufs_recv):
        dist = self.dist
        some = next(iter(bufs_send[0].values()), None)
        if some is not None and some.is_cuda and dist.get_backend(self.device_group) == "gloo":
            # debug transport (several ranks sharing one GPU, no RCCL): stage through pinned host copies
            import torch
            hs = {q: t.cpu() for q, t in bufs_send[0].items()}
            hr = {q: torch.empty(t.shape, dtype=t.dtype) for q, t in bufs_recv[0].items()}
            reqs = [dist.isend(t, q, group=self.device_group) for q, t in hs.items()]
            reqs += [dist.irecv(t, q, group=self.device_group) for q, t in hr.items()]
            for r in reqs:
                r.wait()
            for q, t in bufs_recv[0].items():
                t.copy_(hr[q])
            return
        ops = []
        for q, t in bufs_send[0].items():
            ops.append(dist.P2POp(dist.isend, t, q, group=self.device_group))
        for q, t in bufs_recv[0].items():
            ops.append(dist.P2POp(dist.irecv, t, q, group=self.device_group))
        if ops:
            for w in dist.batch_isend_irecv(ops):
                w.wait()          # stream-ordered for nccl; blocking for gloo

    def allgather_tensor(self, parts, outs, counts):
        import torch
        dist = self.dist
        m = max(counts)
        p = parts[0]
        if p.is_cuda and dist.get_backend(self.device_group) == "gloo":
            lst = [None] * self.size
            dist.all_gather_object(lst, p[:counts[self.rank]].cpu().numpy(), group=self.device_group)
            outs[0].copy_(torch.from_numpy(np.concatenate(lst)))
            return
        if p.numel() != m:
            pad = torch.zeros(m, dtype=p.dtype, device=p.device)
            pad[:p.numel()].copy_(p)
            p = pad
        buf = torch.empty(m * self.size, dtype=p.dtype, device=p.device)
        dist.all_gather_into_tensor(buf, p, group=self.device_group)
        # compact the padded pieces with ONE gather (index cached per layout) instead of one copy kernel per rank
        key = (tuple(counts), str(p.device))
        cache = self.__dict__.setdefault("_ag_index", {})
        if key not in cache:
            cache[key] = torch.from_numpy(compaction_index(counts, m)).to(p.device)
        torch.index_select(buf, 0, cache[key], out=outs[0])

    def barrier(self):
        self.dist.barrier()


# ------------------------------------------------------------------------------------------------------------
# box partition of a structured grid, owned-row assembly
# ------------------------------------------------------------------------------------------------------------

def proc_grid(nranks, dim=3):
    """factor nranks into a box of ranks, first axes first: 2 -> (2,1,1), 4 -> (2,2,1), 8 -> (2,2,2)"""
    g = [1] * dim
    n, d = nranks, 0
    while n > 1:
        for f in (2, 3, 5, 7):
            if n % f == 0:
                g[d % dim] *= f
                n //= f
                break
        else:
            g[d % dim] *= n
            n = 1
        d += 1
    return tuple(g)


def _splitmix(z):
    z = (z + np.uint64(0x9E3779B97F4A7C15))
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def hashed_coords(lo, hi, gshape, jitter, seed):
    """coordinates of the vertices [lo, hi) of the global grid; interior vertices are displaced by a counter-based
    hash of (seed, global id, axis), so every rank computes identical positions for shared ghosts"""
    dim = len(gshape)
    axes = [np.arange(lo[d], hi[d], dtype=np.int64) for d in range(dim)]
    idx = np.meshgrid(*axes, indexing="ij")
    gid = np.zeros(idx[0].shape, dtype=np.int64)
    interior = np.ones(idx[0].shape, dtype=bool)
    for d in range(dim):
        gid = gid * gshape[d] + idx[d]
        interior &= (idx[d] > 0) & (idx[d] < gshape[d] - 1)
    X = np.empty(idx[0].shape + (dim,))
    with np.errstate(over="ignore"):
        for d in range(dim):
            h = 1.0 / (gshape[d] - 1)
            u = _splitmix(gid.astype(np.uint64) * np.uint64(dim) + np.uint64(d) + np.uint64(seed) * np.uint64(0x100000001B3))
            r = (u >> np.uint64(11)).astype(np.float64) * (2.0 / 9007199254740992.0) - 1.0
            X[..., d] = idx[d] * h + jitter * h * r * interior
    return X


class RankState:
    """what one rank holds for one distributed level"""
    pass


def _vexp(idx, bs):
    """scalar indices of the block rows idx (AoS: entry = bs * dof + comp)"""
    idx = np.asarray(idx, dtype=np.int64)
    if bs == 1:
        return idx
    return (idx[:, None] * bs + np.arange(bs)[None, :]).reshape(-1)


def grid_cuts(pgrid, gshape):
    """balanced split of a global vertex grid over a box of ranks: cuts[d][i] = first vertex of rank coordinate i along axis d
    (rank coordinate i owns [cuts[d][i], cuts[d][i + 1])); equal boxes when gshape[d] is a multiple of pgrid[d]"""
    return [np.asarray([(i * int(gshape[d])) // int(pgrid[d]) for i in range(int(pgrid[d]) + 1)], dtype=np.int64) for d in range(len(pgrid))]


def _assemble_owned(rank, pgrid, box, kind, bs, mu, lam, dirichlet, jitter, seed, extent=None, gshape=None, coords="hash"):
    """Rows of the global P1 matrix (kind 0: Poisson, 1: elasticity, 2: elasticity with rotations) owned by `rank`, columns
    [owned | ghost].  Either every rank holds a box of `box` vertices (global grid = pgrid * box: weak scaling), or the
    global grid `gshape` is given and split into balanced, possibly unequal boxes (grid_cuts: strong scaling of ONE problem).
    coords: "hash" = counter-based jitter (hashed_coords: no rank needs more than its own box); "rng" = the positions of
    fem.poisson_fast / elasticity_fast for the same (gshape, jitter, seed), i.e. exactly the single-GPU problem, cut into
    pieces.  Block problems are held as scalar CSR with AoS numbering."""
    dim = len(pgrid)
    if gshape is None:
        gshape = tuple(int(pgrid[d]) * int(box[d]) for d in range(dim))
    gshape = tuple(int(g) for g in gshape)
    cuts = grid_cuts(pgrid, gshape)
    pc = np.unravel_index(rank, pgrid)
    lo = [int(cuts[d][pc[d]]) for d in range(dim)]
    hi = [int(cuts[d][pc[d] + 1]) for d in range(dim)]
    box = tuple(hi[d] - lo[d] for d in range(dim))
    elo = [max(0, lo[d] - 1) for d in range(dim)]
    ehi = [min(gshape[d], hi[d] + 1) for d in range(dim)]
    eshape = tuple(ehi[d] - elo[d] for d in range(dim))
    if coords == "rng":
        from .fem import _jittered_coords
        X = np.ascontiguousarray(_jittered_coords(gshape, jitter, seed)[tuple(slice(elo[d], ehi[d]) for d in range(dim))])
    else:
        X = hashed_coords(elo, ehi, gshape, jitter, seed)
    if extent is not None:
        X = X * np.asarray(extent, dtype=float)
    ne = int(np.prod(eshape))
    coords = np.ascontiguousarray(X.reshape(ne, dim))
    lib = _lib.host()
    shp = np.asarray(eshape, dtype=np.int64)
    rowptr = np.empty(ne + 1, dtype=np.int64)
    _lib.hcheck(lib.amgh_kuhn_pattern(dim, _lib.ptr(shp, C.c_int64), _lib.ptr(rowptr, C.c_int64)))
    nnz = int(rowptr[-1])
    col = np.empty(nnz, dtype=np.int32)
    val = np.empty(nnz * bs * bs)
    _lib.hcheck(lib.amgh_kuhn_assemble(dim, _lib.ptr(shp, C.c_int64), _lib.ptr(coords, C.c_double), int(kind), int(bs), float(mu), float(lam), None,
                                       _lib.ptr(rowptr, C.c_int64), _lib.ptr(col, C.c_int32), _lib.ptr(val, C.c_double), None))
    if bs == 1:
        A_ext = sp.csr_matrix((val, col, rowptr), shape=(ne, ne))
    else:
        A_ext = sp.bsr_matrix((val.reshape(nnz, bs, bs), col, rowptr), shape=(ne * bs, ne * bs)).tocsr()
    Pat = sp.csr_matrix((np.ones(nnz), col, rowptr), shape=(ne, ne))          # vertex graph
    # owned vertices inside the extended box, lexicographic
    eidx = np.arange(ne).reshape(eshape)
    sl = tuple(slice(lo[d] - elo[d], hi[d] - elo[d]) for d in range(dim))
    owned_e = eidx[sl].reshape(-1)
    n_own = owned_e.size
    used = np.unique(Pat[owned_e].indices)
    is_owned = np.zeros(ne, dtype=bool)
    is_owned[owned_e] = True
    ghost_e = used[~is_owned[used]]
    # owner and owner-local (lexicographic in the owner's own box) index of every ghost
    gcoord = np.stack(np.unravel_index(ghost_e, eshape), axis=1) + np.asarray(elo)
    gpc = np.stack([np.searchsorted(cuts[d], gcoord[:, d], side="right") - 1 for d in range(dim)], axis=1) if ghost_e.size else np.zeros((0, dim), dtype=np.int64)
    g_owner = np.ravel_multi_index(tuple(gpc.T), pgrid) if ghost_e.size else np.zeros(0, dtype=np.int64)
    g_rindex = np.zeros(ghost_e.size, dtype=np.int64)
    for d in range(dim):
        olo, ohi = cuts[d][gpc[:, d]], cuts[d][gpc[:, d] + 1]
        g_rindex = g_rindex * (ohi - olo) + (gcoord[:, d] - olo)
    order = np.lexsort((g_rindex, g_owner))
    ghost_e, g_owner, g_rindex = ghost_e[order], g_owner[order], g_rindex[order]
    newidx = np.full(ne, -1, dtype=np.int64)
    newidx[owned_e] = np.arange(n_own)
    newidx[ghost_e] = n_own + np.arange(ghost_e.size)
    A_rows = sp.csr_matrix(A_ext[_vexp(owned_e, bs)])    # complete rows (all cells around an owned vertex are in the ext box)
    cv, cc = np.divmod(A_rows.indices, bs)
    A_loc = sp.csr_matrix((A_rows.data, newidx[cv] * bs + cc, A_rows.indptr), shape=(n_own * bs, (n_own + ghost_e.size) * bs))
    A_loc.sort_indices()
    ocoord = np.stack(np.unravel_index(owned_e, eshape), axis=1) + np.asarray(elo)
    free = np.ones(n_own, dtype=np.uint8)
    names = {"left": (0, 0), "right": (0, gshape[0] - 1), "bottom": (dim - 1, 0), "top": (dim - 1, gshape[dim - 1] - 1)}
    if dim == 3:
        names.update({"front": (1, 0), "back": (1, gshape[1] - 1)})
    for nm in (dirichlet.split("|") if dirichlet else []):
        ax, v = names[nm]
        free[ocoord[:, ax] == v] = 0
    st = RankState()
    st.rank, st.n, st.bs = rank, n_own, int(bs)
    st.A = A_loc
    st.free = free
    st.coords = coords[owned_e]
    st.ghost_owner, st.ghost_rindex = g_owner.astype(np.int64), g_rindex.astype(np.int64)
    st.gshape, st.box, st.lo = gshape, box, lo
    return st


def assemble_poisson_owned(rank, pgrid, box, dirichlet="right|top", jitter=0.2, seed=1, gshape=None, coords="hash"):
    """Rows of the global P1 Poisson matrix owned by `rank`, columns [owned | ghost]: a box of `box` vertices per rank, or
    (gshape given, box ignored) this rank's piece of the balanced split of ONE global grid"""
    return _assemble_owned(rank, pgrid, box, 0, 1, 1.0, 0.0, dirichlet, jitter, seed, gshape=gshape, coords=coords)


def assemble_elasticity_owned(rank, pgrid, box, rotations=False, mu=1.0, lam=0.5, dirichlet="left", jitter=0.2, seed=1, extent=None,
                              gshape=None, coords="hash"):
    """The same for 3D / 2D linear elasticity: dim x dim blocks, or (dim + nrot)^2 blocks with rotational dofs
    (the model problems of ngsamg_amd.fem.elasticity_fast); the state carries bs and is used with energy = 1"""
    dim = len(pgrid)
    bs = dim + (dim * (dim - 1) // 2 if rotations else 0)
    return _assemble_owned(rank, pgrid, box, 2 if rotations else 1, bs, mu, lam, dirichlet, jitter, seed, extent, gshape=gshape, coords=coords)


# ------------------------------------------------------------------------------------------------------------
# distributed setup
# ------------------------------------------------------------------------------------------------------------

def _mat(A, br=1, bc=None):
    """host (block-)CSR Matrix from a scalar scipy matrix with AoS numbering (br x bc blocks, every touched block stored fully)"""
    bc = br if bc is None else bc
    A = sp.csr_matrix(A)
    A.sort_indices()
    if br == 1 and bc == 1:
        return Matrix(A.shape[0], A.shape[1], 1, 1, A.indptr.astype(np.int64), A.indices.astype(np.int32, copy=False), A.data)
    B = sp.bsr_matrix(A, blocksize=(br, bc))
    B.sort_indices()
    return Matrix(A.shape[0] // br, A.shape[1] // bc, br, bc, B.indptr.astype(np.int64), B.indices.astype(np.int32, copy=False), B.data)


def _bs(s):
    return int(getattr(s, "bs", 1))


_DEVICE_SPMM_MIN_ROWS = int(os.environ.get("NGSAMG_DEVICE_SETUP_MIN_ROWS", "20000"))


def _spmm(A, B, br=1, bk=1, bc=1):
    """C = A B through the host library (OpenMP Gustavson, sorted columns).  A has br x bk blocks, B bk x bc blocks (scalar
    scipy matrices in AoS numbering): the product runs on the block matrices -- one index operation per block instead of per
    entry (36x fewer for the 6 x 6 levels; it was the largest single cost of the distributed elasticity setup)"""
    lib = _lib.host()
    MA, MB = _mat(A, br, bk), _mat(B, bk, bc)
    if MA.n_rows >= _DEVICE_SPMM_MIN_ROWS and br * bc <= 36 and _lib.device_setup():
        # products of the big levels on the device (amgx_spgemm: the same bits as the host product)
        from .device import device_spmm
        Cd = device_spmm(MA, MB)
        if Cd is not None:
            if br == 1 and bc == 1:
                return sp.csr_matrix((Cd.val, Cd.col, Cd.rowptr), shape=(MA.n_rows, MB.n_cols))
            return sp.bsr_matrix((np.asarray(Cd.val).reshape(-1, br, bc), Cd.col, Cd.rowptr), shape=(MA.n_rows * br, MB.n_cols * bc)).tocsr()
    da, db = MA.desc(), MB.desc()
    rp = np.zeros(MA.n_rows + 1, dtype=np.int64)
    _lib.hcheck(lib.amgh_matmul(C.byref(da), C.byref(db), _lib.ptr(rp, C.c_int64), None, None))
    col = np.zeros(rp[-1], dtype=np.int32)
    val = np.zeros(rp[-1] * br * bc)
    _lib.hcheck(lib.amgh_matmul(C.byref(da), C.byref(db), _lib.ptr(rp, C.c_int64), _lib.ptr(col, C.c_int32), _lib.ptr(val, C.c_double)))
    if br == 1 and bc == 1:
        return sp.csr_matrix((val, col, rp), shape=(MA.n_rows, MB.n_cols))
    return sp.bsr_matrix((val.reshape(-1, br, bc), col, rp), shape=(MA.n_rows * br, MB.n_cols * bc)).tocsr()


def _peer_segments(owner):
    """ghosts are sorted by owner: {peer: (start, stop)}"""
    seg = {}
    if owner.size:
        peers, starts = np.unique(owner, return_index=True)
        stops = list(starts[1:]) + [owner.size]
        for q, a, b in zip(peers, starts, stops):
            seg[int(q)] = (int(a), int(b))
    return seg


def interior_first(s):
    """Renumber the owned vertices of a rank: [interior | boundary], interior = the row has no ghost column.  Kernels on
    the interior rows then run while the halo exchange is in flight (the reference splits its local rows for the same
    purpose: split_ind, gssmoother.cpp:664-678; stages in hybrid_base_smoother.cpp:501-574).  The peers still address
    this rank's vertices by the old numbers; _send_lists(..., translate=True) settles that."""
    A = sp.csr_matrix(s.A)
    n, bs = s.n, _bs(s)
    rows = np.repeat(np.arange(n * bs), np.diff(A.indptr)) // bs
    has_ghost = np.zeros(n, dtype=bool)
    has_ghost[rows[A.indices >= n * bs]] = True
    perm = np.concatenate([np.nonzero(~has_ghost)[0], np.nonzero(has_ghost)[0]])        # new -> old
    iperm = np.empty(n, dtype=np.int64)
    iperm[perm] = np.arange(n)
    colmap = _vexp(np.concatenate([iperm, n + np.arange(A.shape[1] // bs - n)]), bs)
    A2 = sp.csr_matrix(A[_vexp(perm, bs)])
    A2 = sp.csr_matrix((A2.data, colmap[A2.indices], A2.indptr), shape=A.shape)
    A2.sort_indices()
    s.A = A2
    if getattr(s, "G_abs_partial", None) is not None:      # rows follow, the ghost columns keep their order
        s.G_abs_partial = sp.csr_matrix(sp.csr_matrix(s.G_abs_partial)[_vexp(perm, bs)])
    s.free = np.ascontiguousarray(s.free[perm])
    if getattr(s, "coords", None) is not None:
        s.coords = np.ascontiguousarray(s.coords[perm])
    s.n_interior = int((~has_ghost).sum())
    s.iperm = iperm
    s.perm0 = perm if getattr(s, "perm0", None) is None else s.perm0[perm]     # new -> the caller's original numbering
    return s


def _send_lists(comm, states, translate=False):
    """every rank tells the owners which of their vertices it ghosts -> owners' send lists (symmetric peers).
    translate: the owners were renumbered after the ghost tables were made (interior_first): the requests arrive in the
    owners' old numbers, the owners answer with the new ones"""
    sends = []
    for s in states:
        d = {q: s.ghost_rindex[a:b].astype(np.int64) for q, (a, b) in _peer_segments(s.ghost_owner).items()}
        sends.append(d)
    # make the exchange symmetric: a peer I need nothing from may still need something from me
    recvs = comm.exchange(_symmetrise(comm, states, sends, np.int64))
    for s, r in zip(states, recvs):
        ip = getattr(s, "iperm", None) if translate else None
        s.send = {q: (ip[v] if ip is not None else v) for q, v in r.items() if v.size}
        s.recv_seg = _peer_segments(s.ghost_owner)
    if translate:
        back = comm.exchange(_symmetrise(comm, states, [dict(s.send) for s in states], np.int64))
        for s, r in zip(states, back):
            for q, (a, b) in s.recv_seg.items():
                if r[q].size != b - a:
                    raise NgsAMGError("renumbered ghost table: size mismatch")
                s.ghost_rindex[a:b] = r[q]
            s.iperm = None
    for s in states:
        if not hasattr(s, "n_interior"):
            s.n_interior = 0


def _symmetrise(comm, states, sends, dtype):
    """add empty messages so that `q in sends[p]` <=> `p in sends[q]` (all ranks learn the peer graph by allgather)"""
    pairs = comm.allgather([[(s.rank, q) for q in d] for s, d in zip(states, sends)])[0]
    need = set()
    for lst in pairs:
        for p, q in lst:
            need.add((p, q))
            need.add((q, p))
    out = []
    for s, d in zip(states, sends):
        d = dict(d)
        for p, q in need:
            if p == s.rank and q not in d:
                d[q] = np.empty(0, dtype=dtype)
        out.append(d)
    return out


def _exchange_ghost_values(comm, states, owned_vals):
    """owner -> ghosts for a per-vertex array, 1-D or [n, k] (setup-time, host)"""
    k = owned_vals[0].shape[1:] if owned_vals[0].ndim > 1 else ()
    dt = owned_vals[0].dtype
    sends = [{q: np.ascontiguousarray(v[idx]).reshape(-1) for q, idx in s.send.items()} for s, v in zip(states, owned_vals)]
    sends = _symmetrise(comm, states, sends, dt)
    recvs = comm.exchange(sends)
    outs = []
    for s, r in zip(states, recvs):
        g = np.zeros((s.ghost_owner.size,) + k, dtype=dt)
        for q, (a, b) in s.recv_seg.items():
            g[a:b] = r[q].reshape((b - a,) + k)
        outs.append(g)
    return outs


def _take_rows(indptr, idx):
    """positions of the entries of the rows idx of a CSR structure, row after row"""
    idx = np.asarray(idx, dtype=np.int64)
    lens = (indptr[idx + 1] - indptr[idx]).astype(np.int64)
    tot = int(lens.sum())
    if tot == 0:
        return lens, np.empty(0, dtype=np.int64)
    start = np.repeat(indptr[idx] - np.concatenate([[0], np.cumsum(lens)[:-1]]), lens)
    return lens, start + np.arange(tot)


_SETUP_ONLY_KEYS = ("dist_min_rows", "gs_stage_min_rows", "energy")


def coarsen_distributed_level(comm, states, dim, first, opts):
    """one distributed coarsening step: local aggregation + prolongation, halo of P rows, Galerkin product.
    Block levels (elasticity: opts["energy"] = 1) are handled through their scalar CSR images; the prolongation travels
    as block rows (fine block size bf, coarse block size bc = dim + nrot)."""
    o = dict(opts)
    energy = int(o.get("energy", 0))
    nxt = []
    P_blk = []
    stuck = False
    for s in states:
        bf = _bs(s)
        if s.n == 0:
            # a rank without rows (NGSolve's master rank holds no mesh in classic MPI runs; the reference guards its
            # smoothers with `if (A.Height())`): it takes part in every collective with empty pieces
            bc = 1 if energy == 0 else (6 if dim == 3 else 3)
            c = RankState()
            c.rank, c.n, c.bs, c.n_interior = s.rank, 0, bc, 0
            c.coords = None if s.coords is None else np.zeros((0, np.asarray(s.coords).shape[1] if np.asarray(s.coords).ndim == 2 else dim))
            c.free = np.zeros(0, dtype=np.uint8)
            s.agg = np.zeros(0, dtype=np.int32)
            P_blk.append((np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros((0, bf, bc)), bf, bc))
            nxt.append(c)
            continue
        A_oo = sp.csr_matrix(s.A[:, :s.n * bf])
        kw = dict(o)
        dflt = (0.05 if dim == 3 else 0.1) if energy == 0 else (0.1 if dim == 3 else 0.15)
        kw["first_aaf"] = o.get("first_aaf", dflt) if first else o.get("aaf", 2.0 ** -dim)
        kw["max_levels"] = 2
        kw["max_coarse_size"] = 1
        if not int(kw.get("enable_multistep", 0)):
            kw["prol_only"] = 1   # one step, P only: the coarse operator is formed below with the halo rows of P
        # prolongation rule: the reference smooths vertices shared between ranks with the replacement matrix only
        # (get_cols_classic: "if (eqc != 0) return false", vertex_factory_impl.hpp:1920); the rank-local setup sees the owned x owned
        # block of A, whose rows at the interface are incomplete, so every row takes that branch here (aux_smoothed)
        if "prol_type" not in kw:
            kw["prol_type"] = 1 if int(kw.get("spw", 1)) else 3
        H = Hierarchy(_mat(A_oo, bf), s.free, s.coords, dim=dim, energy=energy, **{k: v for k, v in kw.items() if k not in _SETUP_ONLY_KEYS})
        if H.n_levels < 2:
            stuck = True
            H = None
            break
        PM = H.levels[0].P
        bc = PM.bc
        agg = np.array(H.levels[0].agg, copy=True)        # blocks of the block smoother (never cross ranks)
        c = RankState()
        c.rank, c.n, c.bs = s.rank, PM.n_cols, bc
        c.coords = H.levels[1].coords.copy() if H.levels[1].coords is not None else None
        # coarse numbering [interior | boundary]: a coarse row can only reach a coarse ghost through a fine row that has a
        # ghost column, so "some fine vertex of my prolongation column is a boundary row" is a safe boundary test
        Af = sp.csr_matrix(s.A)
        frows = np.repeat(np.arange(s.n * bf), np.diff(Af.indptr)) // bf
        bnd_f = np.zeros(s.n, dtype=np.float64)
        bnd_f[frows[Af.indices >= s.n * bf]] = 1.0
        Pat = sp.csr_matrix((np.ones(PM.col.size), PM.col, PM.rowptr), shape=(s.n, c.n))
        bnd_c = (Pat.T @ bnd_f) > 0
        permc = np.concatenate([np.nonzero(~bnd_c)[0], np.nonzero(bnd_c)[0]])
        ipermc = np.empty(c.n, dtype=np.int64)
        ipermc[permc] = np.arange(c.n)
        Pb = sp.bsr_matrix((PM.val.reshape(-1, bf, bc).copy(), ipermc[PM.col], PM.rowptr.copy()), shape=(s.n * bf, c.n * bc))
        Pb.sort_indices()
        if c.coords is not None:
            c.coords = np.ascontiguousarray(c.coords[permc])
        c.n_interior = int((~bnd_c).sum())
        s.agg = np.where(agg >= 0, ipermc[np.maximum(agg, 0)], -1).astype(np.int32)
        P_blk.append((Pb.indptr.astype(np.int64), Pb.indices.astype(np.int64), np.asarray(Pb.data), bf, bc))
        c.free = np.ones(c.n, dtype=np.uint8)
        nxt.append(c)
    # a rank whose local coarsening made no progress must not leave the others waiting in the next collective: agree first
    if any(comm.allgather([stuck for _ in states])[0]):
        raise NgsAMGError("distributed coarsening got stuck on a rank (raise dist_min_rows or lower max_dist_levels)")
    # P rows of the ghost vertices: owners send (row lengths, coarse ids at the owner, blocks) for their send lists
    cnt_s, col_s, val_s = [], [], []
    for s, (ip, ix, dat, bf, bc) in zip(states, P_blk):
        dc, dcol, dval = {}, {}, {}
        for q, idx in s.send.items():
            lens, sel = _take_rows(ip, idx)
            dc[q] = lens
            dcol[q] = ix[sel].astype(np.int64)
            dval[q] = np.ascontiguousarray(dat[sel], dtype=np.float64).reshape(-1)
        cnt_s.append(dc)
        col_s.append(dcol)
        val_s.append(dval)
    cnt_r = comm.exchange(_symmetrise(comm, states, cnt_s, np.int64))
    col_r = comm.exchange(_symmetrise(comm, states, col_s, np.int64))
    val_r = comm.exchange(_symmetrise(comm, states, val_s, np.float64))
    for s, c, (ip, ix, dat, bf, bc), cr, lr, vr in zip(states, nxt, P_blk, cnt_r, col_r, val_r):
        peers = sorted(s.recv_seg, key=lambda q: s.recv_seg[q][0])      # ghost order = peer order
        # coarse ghosts: unique (owner, coarse id at owner), sorted by (owner, id)
        own, rid = [], []
        for q in sorted(peers):
            ids = np.unique(lr[q])
            own.append(np.full(ids.size, q, dtype=np.int64))
            rid.append(ids)
        c.ghost_owner = np.concatenate(own) if own else np.empty(0, dtype=np.int64)
        c.ghost_rindex = np.concatenate(rid) if rid else np.empty(0, dtype=np.int64)
        seg = _peer_segments(c.ghost_owner)
        ng = s.ghost_owner.size
        ncx = c.n + c.ghost_owner.size
        lens = np.zeros(ng, dtype=np.int64)
        cols, vals = [], []
        for q in peers:
            a, b = s.recv_seg[q]
            if cr[q].size != b - a:
                raise NgsAMGError("halo of P rows: size mismatch")
            lens[a:b] = cr[q]
            ga, gb = seg.get(q, (0, 0))
            cols.append(c.n + ga + np.searchsorted(c.ghost_rindex[ga:gb], lr[q]))
            vals.append(vr[q])
        rows_ptr = np.concatenate([[0], np.cumsum(lens)])
        gcols = np.concatenate(cols) if cols else np.empty(0, dtype=np.int64)
        gvals = (np.concatenate(vals) if vals else np.empty(0)).reshape(-1, bf, bc)
        P_gh = sp.bsr_matrix((gvals, gcols, rows_ptr), shape=(ng * bf, ncx * bc)).tocsr()
        P_own_ext = sp.bsr_matrix((dat, ix, ip), shape=(s.n * bf, ncx * bc)).tocsr()
        P_ext = sp.vstack([P_own_ext, P_gh], format="csr")
        P = sp.csr_matrix(sp.bsr_matrix((dat, ix, ip), shape=(s.n * bf, c.n * bc)))
        AP = _spmm(s.A, P_ext, bf, bf, bc)
        c.A = _spmm(sp.csr_matrix(P.T), AP, bc, bf, bc)
        c.A.sort_indices()
        s.AP, s.P_own_ext = AP, P_own_ext          # for the folded prolongation Q = P - w Dinv (A P), see _fold
        s.P = P
        s.P.sort_indices()
        s.PT = sp.csr_matrix(P.T)
        s.PT.sort_indices()
        s.bs_c = bc
    _send_lists(comm, nxt)
    return nxt


def _block_dinv(A_oo, bs, free, pinv):
    """inverted block diagonal through the host library (gssmoother.cpp:143-170 incl. the pseudo-inverse rule)"""
    lib = _lib.host()
    M = _mat(A_oo, bs)
    d = M.desc()
    out = np.zeros(M.n_rows * bs * bs)
    fr = np.ascontiguousarray(free, dtype=np.uint8)
    _lib.hcheck(lib.amgh_calc_dinv(C.byref(d), _lib.ptr(fr, C.c_uint8), int(bool(pinv)), _lib.ptr(out, C.c_double)))
    return out.reshape(M.n_rows, bs * bs)


def _dinv_ext(comm, states, pinv=False):
    dins = []
    for s in states:
        bs = _bs(s)
        if bs == 1:
            d = s.A[:, :s.n].diagonal()
            di = np.where(s.free.astype(bool), 1.0 / np.where(d != 0, d, 1.0), 0.0)
        else:
            di = _block_dinv(sp.csr_matrix(s.A[:, :s.n * bs]), bs, s.free, pinv)
        dins.append(di)
    gh = _exchange_ghost_values(comm, states, dins)
    for s, di, g in zip(states, dins, gh):
        s.dinv_ext = np.concatenate([di, g]).reshape(-1)


def _fold(states, omega):
    """Q = (I - omega Dinv A) P on the owned rows, columns = coarse [owned | ghost]: the Jacobi post-smoothing folded
    into the prolongation (amgx.h: amgx_level_desc.Q, amgx_cycle_up).  A P is a by-product of the Galerkin product."""
    for s in states:
        wd = omega * s.dinv_ext[:s.n]
        Q = sp.csr_matrix(s.P_own_ext - sp.diags(wd) @ s.AP)
        Q.sort_indices()
        s.Q = Q
        del s.AP, s.P_own_ext


def _hybrid_gs_data(comm, states):
    """per level: inverse of the modified diagonal md = max(1, 0.51 (1 + ad)) d with ad_k = sum over the off-rank
    couplings |g_kj| / sqrt(d_k d_j)  (reference hybrid_smoother_utils.hpp:35-142), and a colouring of the
    rank-local (owned x owned) graph for the multicolour sweep.
    Block levels (hybrid_smoother_utils.hpp:55-68, 86-98, 128-141): ad_k(l) = sum_j sum_m |g_kj(l, m)| / sqrt(d_k(l, l) d_j(m, m)),
    md_k = max(1, max_l 0.51 (1 + ad_k(l))) d_k, so the inverse is the (pseudo-)inverse of _dinv_ext divided by that factor."""
    lib = _lib.host()
    bs = _bs(states[0])
    diags = [np.asarray(sp.csr_matrix(s.A)[:, :s.n * bs].diagonal()).reshape(s.n, bs) for s in states]
    gdiag = _exchange_ghost_values(comm, states, diags)
    for s, d, gd in zip(states, diags, gdiag):
        d, gd = d.reshape(-1), gd.reshape(-1)
        A = sp.csr_matrix(s.A)
        G = abs(sp.csr_matrix(A[:, s.n * bs:]))
        Gp = getattr(s, "G_abs_partial", None)       # level 0 of a bridged hierarchy: sum over the ranks of |partial g| (bridge.py)
        if Gp is not None and Gp.shape == G.shape:
            G = sp.csr_matrix(Gp)
        free = np.repeat(s.free.astype(bool), bs)
        sd = np.sqrt(np.where(d > 0, d, 1.0))
        sg = np.sqrt(np.where(gd > 0, gd, 1.0))
        ad = np.asarray(G.multiply(1.0 / sd[:, None]).multiply(1.0 / sg[None, :]).sum(axis=1)).ravel() if G.shape[1] else np.zeros(s.n * bs)
        if bs == 1:
            md = np.maximum(1.0, 0.51 * (1.0 + ad)) * d
            dinv = np.where(free & (md != 0), 1.0 / np.where(md != 0, md, 1.0), 0.0)
        else:
            fac = np.maximum(1.0, (0.51 * (1.0 + np.where(free, ad, 0.0))).reshape(s.n, bs).max(axis=1))
            dinv = (s.dinv_ext[:s.n * bs * bs].reshape(s.n, bs * bs) / fac[:, None]).reshape(-1)
        s.dinv_gs_ext = np.concatenate([dinv, np.zeros(s.ghost_owner.size * bs * bs)])
        Aoo = _mat(sp.csr_matrix(A[:, :s.n * bs]), bs)
        color = np.zeros(s.n, dtype=np.int32)
        nc = C.c_int32()
        dsc = Aoo.desc()
        fr = np.ascontiguousarray(s.free, dtype=np.uint8)
        _lib.hcheck(lib.amgh_coloring(C.byref(dsc), _lib.ptr(fr, C.c_uint8), _lib.ptr(color, C.c_int32), C.byref(nc)))
        s.color, s.n_colors = color, int(nc.value)


def _hybrid_gsb_data(comm, states, block_rows=None):
    """block-hybrid Gauss-Seidel on a rank-partitioned level (amgx_level_desc.gs_block_rows): blocks of B consecutive owned
    rows; blocked colouring; inverse of the l1-modified diagonal whose off-block weight includes the couplings to ghost
    columns (their diagonal entries come from the owners)"""
    from .device import gs_block_rows
    lib = _lib.host()
    bs = _bs(states[0])
    if bs > 1:
        return _hybrid_bgsb_data(comm, states, block_rows)
    diags = [np.asarray(s.A[:, :s.n].diagonal()) for s in states]
    gdiag = _exchange_ghost_values(comm, states, diags)
    Bs = []
    for s in states:
        M = _mat(s.A)
        if block_rows:
            # a caller's block size is capped by what the longest row allows: G lanes share a row (16 entries each, + 1 for G = 1)
            # and a workgroup has at most 1024 lanes (build_gsb)
            mx = int(np.diff(M.rowptr).max()) if M.n_rows else 0
            G = next((g for g in (1, 2, 4, 8, 16) if mx <= 16 * g + (1 if g == 1 else 0)), 0)
            Bs.append(min(int(block_rows), 1024 // G) if G else 0)
        else:
            Bs.append(gs_block_rows(M))
    votes = [x for lst in comm.allgather([b if s.n > 0 else -1 for b, s in zip(Bs, states)]) for x in lst if x >= 0]
    B = min(votes) if votes else 0                       # (0 if any non-empty rank cannot use the block form)
    for s, gd in zip(states, gdiag):
        if B <= 0:
            raise NgsAMGError("hgs: a rank-partitioned level cannot use the block-hybrid form (rows too long or level too small); use sm_type = gs")
        M = _mat(s.A)
        d = M.desc()
        fr = np.ascontiguousarray(s.free, dtype=np.uint8)
        color = np.full(s.n, -1, dtype=np.int32)
        nc = C.c_int32()
        _lib.hcheck(lib.amgh_coloring_blocked(C.byref(d), _lib.ptr(fr, C.c_uint8), B, _lib.ptr(color, C.c_int32), C.byref(nc)))
        dinv = np.zeros(M.n_cols)
        gd = np.ascontiguousarray(gd, dtype=np.float64)
        _lib.hcheck(lib.amgh_hybrid_dinv_ext(C.byref(d), _lib.ptr(fr, C.c_uint8), B, _lib.ptr(gd, C.c_double) if gd.size else None, _lib.ptr(dinv, C.c_double)))
        s.color, s.n_colors, s.dinv_gs_ext, s.gs_B = color, int(nc.value), dinv, B
        # the same sweep for the serial oracle / CPU stage backend: visiting order (block, colour), blocks never see each other's updates
        rows = np.nonzero(color >= 0)[0]
        key = (rows // B).astype(np.int64) * (int(nc.value) + 1) + color[rows]
        s.gs_order = rows[np.argsort(key, kind="stable")].astype(np.int32)
        s.gs_blockid = (np.arange(s.n) // B).astype(np.int32)


def _hybrid_bgsb_data(comm, states, block_rows=None):
    """_hybrid_gsb_data for square-block levels (bgsb_sweep_kernel): sweep blocks of BB consecutive owned block rows, blocked
    colouring of the block graph, block diagonal inverse divided by max(1, max_l 0.51 (1 + ad_k(l))) where ad_k(l) sums
    |a_kj(l, m)| / sqrt(d_k(l, l) d_j(m, m)) over every coupling that leaves the sweep block -- to another block of the rank or to
    a ghost column, whose diagonal entries come from the owner (hybrid_smoother_utils.hpp:55-68, 86-98, 128-141 with sweep
    blocks in the role of the reference's ranks)"""
    from .device import gs_block_rows
    lib = _lib.host()
    bs = _bs(states[0])
    diags = [np.asarray(sp.csr_matrix(s.A)[:, :s.n * bs].diagonal()).reshape(s.n, bs) for s in states]
    gdiag = _exchange_ghost_values(comm, states, diags)
    mats = [_mat(s.A, bs) for s in states]
    Bs = [int(block_rows) if block_rows else gs_block_rows(_mat(sp.csr_matrix(s.A)[:, :s.n * bs], bs)) for s in states]
    votes = [x for lst in comm.allgather([b if s.n > 0 else -1 for b, s in zip(Bs, states)]) for x in lst if x >= 0]
    B = min(votes) if votes else 0
    rb = 64 // bs
    B = (B // rb) * rb                                   # a whole number of BSELL slices
    for s, M, d, gd in zip(states, mats, diags, gdiag):
        if B <= 0:
            raise NgsAMGError("hgs: a rank-partitioned block level cannot use the block-hybrid form (level too small); use sm_type = gs")
        dsc = M.desc()
        fr = np.ascontiguousarray(s.free, dtype=np.uint8)
        color = np.full(s.n, -1, dtype=np.int32)
        nc = C.c_int32()
        _lib.hcheck(lib.amgh_coloring_blocked(C.byref(dsc), _lib.ptr(fr, C.c_uint8), B, _lib.ptr(color, C.c_int32), C.byref(nc)))
        A = sp.coo_matrix(sp.csr_matrix(s.A))
        dd = np.concatenate([d.reshape(-1), np.asarray(gd).reshape(-1)])
        bi, bj = A.row // bs, A.col // bs
        leaves = (bj >= s.n) | ((bj // B) != (bi // B))
        dl, dm = dd[A.row], dd[A.col]
        ok = leaves & (dl > 0) & (dm > 0)
        ad = np.bincount(A.row[ok], weights=np.abs(A.data[ok]) / np.sqrt(dl[ok] * dm[ok]), minlength=s.n * bs)
        fac = np.maximum(1.0, np.where(d.reshape(-1) > 0, 0.51 * (1.0 + ad), 0.0).reshape(s.n, bs).max(axis=1))
        fac = np.where(s.free.astype(bool), fac, 1.0)
        dinv = (s.dinv_ext[:s.n * bs * bs].reshape(s.n, bs * bs) / fac[:, None]).reshape(-1)
        s.dinv_gs_ext = np.concatenate([dinv, np.zeros(s.ghost_owner.size * bs * bs)])
        s.color, s.n_colors, s.gs_B = color, int(nc.value), B
        rows = np.nonzero(color >= 0)[0]
        key = (rows // B).astype(np.int64) * (int(nc.value) + 1) + color[rows]
        s.gs_order = rows[np.argsort(key, kind="stable")].astype(np.int32)
        s.gs_blockid = (np.arange(s.n) // B).astype(np.int32)


def _hybrid_bgs_data(states):
    """hybrid block Gauss-Seidel (reference HybridBS, block_gssmoother.cpp:505-585): BSmoother on the rank-local matrix M
    whose diagonal is replaced by the l1-modified one (mod_diag), blocks = local aggregates; needs _hybrid_gs_data first"""
    from .hierarchy import bgs_blocks_from_aggregates, bgs_data
    for s in states:
        Aoo = sp.csr_matrix(s.A[:, :s.n])
        md = np.where(s.dinv_gs_ext[:s.n] != 0, 1.0 / np.where(s.dinv_gs_ext[:s.n] != 0, s.dinv_gs_ext[:s.n], 1.0), Aoo.diagonal())
        Amod = sp.csr_matrix(Aoo - sp.diags(Aoo.diagonal()) + sp.diags(md))
        Amod.sort_indices()
        bp, br = bgs_blocks_from_aggregates(s.agg, s.free)
        s.bgs = bgs_data(_mat(Amod), bp, br, pinv=False)


class _TopHierarchy:
    """duck-typed Hierarchy holding the rank-partitioned levels of one rank (for DeviceAMGMatrix)"""

    def __init__(self, states, gs=False, fold=False, bgs=False):
        self.levels = []
        for i, s in enumerate(states):
            last = i + 1 == len(states)
            use_gs = gs and not last
            color = s.color if use_gs else np.full(s.n, -1, dtype=np.int32)
            dinv = s.dinv_gs_ext if use_gs else s.dinv_ext
            bf = _bs(s)
            bc = int(getattr(s, "bs_c", bf))
            self.levels.append(Level(A=_mat(s.A, bf), P=None if last else _mat(s.P, bf, bc), PT=None if last else _mat(s.PT, bc, bf),
                                     free=s.free, dinv=np.ascontiguousarray(dinv), coords=None, color=color,
                                     n_colors=s.n_colors if use_gs else 0, agg=None,
                                     Q=_mat(s.Q) if (fold and not last and not use_gs) else None,
                                     bgs=s.bgs if (bgs and not last) else None))
            L = self.levels[-1]
            if use_gs and hasattr(s, "gs_B"):
                L.hgs_pre = dict(B=s.gs_B, color=s.color, n_colors=s.n_colors, dinv=s.dinv_gs_ext)
                L.gs_order, L.gs_block = s.gs_order, s.gs_blockid
        self.coarse_n = 0
        self.coarse_inv = np.empty(0)
        self.n_levels = len(self.levels)


class DistributedAMG:
    """Jacobi V(1,1) over rank-partitioned fine levels + replicated coarse hierarchy.

    comm:     LoopbackComm(R) (R virtual ranks in this process) or TorchComm() (one rank per process)
    states0:  level-0 RankState of every local rank (assemble_poisson_owned)
    backend:  callable(top_hierarchy, tail_hierarchy, rank) -> (top_ops, tail_ops); default = the HIP library
    """

    def __init__(self, comm, states0, dim=3, omega=0.9, dist_min_rows=50000, max_dist_levels=3, device=0,
                 backend=None, sm_type="jacobi", fold=True, sm_steps=1, sm_symm=False, mg_cycle="V",
                 cheb_degree=None, cheb_ratio=10.0, cheb_lambda_max=None, **opts):
        if sm_type not in ("jacobi", "gs", "hgs", "bgs", "cheby"):
            raise NgsAMGError("DistributedAMG: sm_type must be jacobi, gs (multicolour stages), hgs (block-hybrid Gauss-Seidel), bgs or cheby")
        if opts.get("jacobi_prec", "double") != "double":
            raise NgsAMGError("DistributedAMG: jacobi_prec (single-precision Jacobi images) is not available on rank-partitioned hierarchies")
        mp = opts.get("mat_prec", "double")
        if any(isinstance(v, str) and v.lower() == "single_gs_all" for v in (mp if isinstance(mp, (list, tuple)) else [mp])):
            raise NgsAMGError("DistributedAMG: mat_prec 'single_gs_all' (single-precision images of scalar Gauss-Seidel levels) is not "
                              "available on rank-partitioned hierarchies")
        # (an opt-in in two words: the type and its degree.  The degree has no default here: it fixes the 2 x degree halo exchanges per
        #  level and application, and a call that names the type alone is refused as it was before the option existed)
        if sm_type == "cheby" and cheb_degree is None:
            raise NgsAMGError("DistributedAMG: sm_type 'cheby' on rank-partitioned levels needs an explicit cheb_degree (1 .. 8): it fixes "
                              "the 2 x degree halo exchanges per level and application")
        if sm_type == "cheby" and backend is not None:
            raise NgsAMGError("DistributedAMG: the Chebyshev smoother runs through the device driver only (backend=None); the stage-by-stage "
                              "Python backend is test infrastructure for Jacobi and Gauss-Seidel")
        self.comm, self.dim, self.omega, self.sm_type = comm, dim, omega, sm_type
        # sm_type = "cheby" (DESIGN.md 5.4, 5.11): one degree and ratio for every level; cheb_lambda_max: None (estimated: collectively
        # on the rank-partitioned levels, by amgx_create in the replicated tail), one value for the rank-partitioned levels, or a
        # list with one entry per rank-partitioned level (the tail is always estimated)
        self.cheb_degree, self.cheb_ratio, self.cheb_lambda_max = cheb_degree, cheb_ratio, cheb_lambda_max
        if sm_type == "cheby":
            from .device import cheby_args
            if isinstance(cheb_degree, (list, tuple, np.ndarray)) or isinstance(cheb_ratio, (list, tuple, np.ndarray)):
                raise NgsAMGError("DistributedAMG: cheb_degree and cheb_ratio are one value for all levels")
            cheby_args(cheb_degree, cheb_ratio, None)
        # energy = 1: linear elasticity (states from assemble_elasticity_owned: block levels, rigid-body prolongation blocks,
        # coarse block size dim + nrot); block levels run block-Jacobi in the literal stage order
        self.energy = int(opts.get("energy", 0))
        blocks = any(_bs(s) > 1 for s in states0) or self.energy == 1
        if blocks and sm_type not in ("jacobi", "gs", "hgs", "cheby"):
            raise NgsAMGError("DistributedAMG: rank-partitioned block levels support sm_type = jacobi | gs | hgs | cheby")
        if blocks and sm_type == "hgs" and backend is not None:
            raise NgsAMGError("DistributedAMG: block-hybrid Gauss-Seidel on block levels runs through the device driver only (backend=None)")
        # fold: Jacobi post-smoothing folded into the prolongation (one product with Q on the way up, one halo exchange
        # per stage); False = the literal stage sequence pre / restrict / prolong / post with two exchanges per level
        # (AMGX_NO_FOLD=1, the switch that makes the single-GPU handle run the literal kernel sequence, selects the literal
        # stages here too: the decision is taken from the environment on every rank alike, before anything is built)
        # ngs_amg_sm_steps / ngs_amg_sm_symm (ProxySmoother, base_smoother.hpp:169-229) and ngs_amg_mg_cycle = "W" on rank-partitioned
        # levels: the native driver's step-by-step cycle (csrc/device/dist.hpp, DistCycle::stepwise); the folded V(1,1) form
        # and the stage-by-stage Python test backend cover sm_steps = 1, sm_symm = False, V only
        self.sm_steps, self.sm_symm, self.mg_cycle = int(sm_steps), bool(sm_symm), str(mg_cycle)
        if self.mg_cycle not in ("V", "W"):
            raise NgsAMGError("DistributedAMG: mg_cycle must be V or W")
        self.generic = self.sm_steps > 1 or self.sm_symm or self.mg_cycle == "W"
        if self.generic and backend is not None:
            raise NgsAMGError("DistributedAMG: sm_steps / sm_symm / W-cycle run through the device driver only (backend=None)")
        self.fold = bool(fold) and sm_type == "jacobi" and not blocks and not os.environ.get("AMGX_NO_FOLD") and not self.generic
        pinv = bool(opts.get("regularize_cmats", self.energy == 1 and all(_bs(s) == dim for s in states0)))
        for s in states0:
            interior_first(s)
        _send_lists(comm, states0, translate=True)
        levels = [states0]
        while len(levels) <= max_dist_levels:
            cur = levels[-1]
            sizes = [x for lst in comm.allgather([s.n for s in cur]) for x in lst if x > 0]       # (empty ranks do not decide)
            gmin = min(sizes) if sizes else 0
            if gmin < dist_min_rows:
                break
            levels.append(coarsen_distributed_level(comm, cur, dim, len(levels) == 1, opts))
        if len(levels) == 1:       # always at least one distributed level
            levels.append(coarsen_distributed_level(comm, levels[0], dim, True, opts))
        for lv in levels:
            _dinv_ext(comm, lv, pinv)
        if sm_type in ("gs", "bgs"):
            for lv in levels[:-1]:
                _hybrid_gs_data(comm, lv)
        if sm_type == "hgs":
            for lv in levels[:-1]:
                _hybrid_gsb_data(comm, lv, opts.get("hgs_block_rows"))
        if sm_type == "gs":
            for lv in levels[:-1]:
                _gs_stages(comm, lv, opts.get("gs_stage_min_rows", 65536))
        if sm_type == "bgs":
            for lv in levels[:-1]:
                _hybrid_bgs_data(lv)
        if self.fold:
            for lv in levels[:-1]:
                _fold(lv, omega)
        self.dist_levels = levels
        self.k = len(levels) - 1                      # levels 0..k-1 are smoothed in distributed form, level k is gathered
        # ---- gather level k and build the replicated tail ---------------------------------------------
        last = levels[-1]
        counts = comm.allgather([s.n for s in last])[0]
        self.counts = [int(c) for c in counts]
        offs = np.concatenate([[0], np.cumsum(self.counts)])
        self.offs = offs
        pieces = []
        bk = _bs(last[0])
        for s in last:
            gmapv = np.concatenate([offs[s.rank] + np.arange(s.n), offs[s.ghost_owner] + s.ghost_rindex]).astype(np.int64)
            A = sp.csr_matrix(s.A)
            cv, cc = np.divmod(A.indices, bk)
            pieces.append((s.rank, A.indptr.copy(), gmapv[cv] * bk + cc, A.data.copy(), None if s.coords is None else np.asarray(s.coords)))
        allp = comm.allgather(pieces)[0]
        allp = sorted(allp, key=lambda t: t[0])
        ntot = int(offs[-1])
        indptr = np.concatenate([[0]] + [np.diff(p[1]) for p in allp]).cumsum()
        Ag = sp.csr_matrix((np.concatenate([p[3] for p in allp]), np.concatenate([p[2] for p in allp]), indptr), shape=(ntot * bk, ntot * bk))
        Ag.sort_indices()
        self.A_tail = Ag
        topts = {k: v for k, v in opts.items() if k not in ("first_aaf",) + _SETUP_ONLY_KEYS}
        topts["first_aaf"] = opts.get("aaf", 2.0 ** -dim)
        coords_g = np.concatenate([p[4] for p in allp]) if (self.energy == 1 and all(p[4] is not None for p in allp)) else None
        self.tail_hier = Hierarchy(_mat(Ag, bk), None, coords_g, dim=dim, energy=self.energy, **topts)
        if sm_type == "hgs":
            # the replicated tail sweeps in the block-hybrid form too (one launch per sweep instead of one per colour):
            # blocks, colours and modified diagonals are fixed here so that every consumer of the hierarchy sees the same data
            from .device import gs_block_rows, hybrid_gs_data
            for L in self.tail_hier.levels[:-1]:
                B = gs_block_rows(L.A)
                if B > 0:
                    col, nc, dinv = hybrid_gs_data(L.A, L.free, B)
                    L.hgs_pre = dict(B=B, color=col, n_colors=nc, dinv=dinv)
                    rows = np.nonzero(col >= 0)[0]
                    key = (rows // B).astype(np.int64) * (nc + 1) + col[rows]
                    L.gs_order = rows[np.argsort(key, kind="stable")].astype(np.int32)
                    L.gs_block = (np.arange(L.A.n_rows) // B).astype(np.int32)
                    L.hgs_dinv = dinv
        if sm_type == "bgs":
            self.tail_hier.build_bgs(pinv=False)
        # ---- per-rank execution objects --------------------------------------------------------------------
        self.tops = [_TopHierarchy([lv[i] for lv in levels], gs=(sm_type in ("gs", "hgs", "bgs")), fold=self.fold, bgs=(sm_type == "bgs"))
                     for i in range(len(states0))]
        self._dev = None
        if backend is None:
            # the product path: the whole collective cycle behind the C ABI (amgx_dist_apply): pack kernels, RCCL (or
            # device copies between virtual ranks), stream overlap -- no Python between the stages
            self._dev = _DeviceDist(self, device)
            self.ops = self._dev.ops
            return
        # stage-by-stage driver for test backends (tests/dist_cpu_backend.py): same tables, same stage order.  It is test
        # infrastructure for boxes WITHOUT a GPU: where a device exists the product path is the native driver above
        # (NGSAMG_STAGE_BACKEND_OK=1 lifts the refusal, e.g. to compare the two on one box)
        try:
            import torch
            has_gpu = torch.cuda.is_available()
        except Exception:
            has_gpu = False
        if has_gpu and not os.environ.get("NGSAMG_STAGE_BACKEND_OK"):
            raise NgsAMGError("DistributedAMG: the stage-by-stage Python backend is the CPU test path; on a GPU box use the native driver "
                              "(backend=None) or set NGSAMG_STAGE_BACKEND_OK=1")
        self.ops = [backend(top, self.tail_hier, i) for i, top in enumerate(self.tops)]
        self._alloc()

    def pcg(self, bs, xs, tol=1e-8, maxsteps=200, use_pre=True, single_reduction=False):
        """collective preconditioned CG on the rank-partitioned level-0 operator with this cycle as preconditioner
        (amgx_dist_pcg; the reference's driver is NGSolve's CGSolver on ParallelVectors, tests/h1/amg_utils.py:337-363).
        bs[i], xs[i]: owned level-0 CUDA tensors of local rank i; xs hold the initial guess.  Returns (iterations, errs)."""
        if self._dev is None:
            raise NgsAMGError("pcg: needs the device driver (no CPU path)")
        return self._dev.pcg(bs, xs, tol=tol, maxsteps=maxsteps, use_pre=use_pre, single_reduction=single_reduction)

    def gmres(self, bs, xs, tol=1e-8, maxsteps=200, restart=30, use_pre=True):
        """collective restarted GMRES(restart) with this cycle as left preconditioner (amgx_dist_gmres)"""
        if self._dev is None:
            raise NgsAMGError("gmres: needs the device driver (no CPU path)")
        return self._dev.gmres(bs, xs, tol=tol, maxsteps=maxsteps, restart=restart, use_pre=use_pre)

    def smoother_info(self, level):
        """the smoother of a level of the whole hierarchy (amgx_smoother_info): levels below k are answered by the top handles of the
        local ranks, which must agree; level k and beyond by the replicated tail"""
        if self._dev is None:
            raise NgsAMGError("smoother_info: needs the device driver")
        if level >= self.k:
            return self.ops[0].tail.smoother_info(level - self.k)
        infos = [op.top.smoother_info(level) for op in self.ops]
        assert all(i == infos[0] for i in infos), f"level {level}: the local ranks disagree on the smoother: {infos}"
        return infos[0]

    def level_k_map(self, i):
        """level k of local rank i in its [owned | ghost] layout -> index in the gathered (replicated) vector"""
        sk = self.dist_levels[self.k][i]
        mv = np.concatenate([self.offs[sk.rank] + np.arange(sk.n), self.offs[sk.ghost_owner] + sk.ghost_rindex]).astype(np.int64)
        return _vexp(mv, _bs(sk))

    # ---------------------------------------------------------------------------------------------------------
    def _alloc(self):
        self.buf = []
        for i, ops in enumerate(self.ops):
            b = {"bext": [], "text": [], "x": [], "r": [], "send": [], "sidx": []}
            for l in range(self.k):
                s = self.dist_levels[l][i]
                bsl = _bs(s)
                next_ = (s.n + s.ghost_owner.size) * bsl
                b["bext"].append(ops.zeros(next_))
                b["text"].append(ops.zeros(next_))
                b["x"].append(ops.zeros(s.n * bsl))
                b["r"].append(ops.zeros(s.n * bsl))
                b.setdefault("xext", []).append(ops.zeros(next_) if (self.sm_type in ("gs", "hgs", "bgs") or self.fold) else None)
                b.setdefault("b", []).append(ops.zeros(s.n * bsl) if self.sm_type in ("gs", "hgs", "bgs") else None)
                # ONE pack per halo: all peers' send lists concatenated; a peer's message is a slice of the buffer
                peers = sorted(s.send)
                allidx = _vexp(np.concatenate([s.send[q] for q in peers]), bsl) if peers else np.empty(0, dtype=np.int64)
                sbuf = ops.zeros(allidx.size)
                off, views = 0, {}
                for q in peers:
                    views[q] = sbuf[off:off + s.send[q].size * bsl]
                    off += s.send[q].size * bsl
                b["send"].append(views)
                b["sidx"].append((ops.index(allidx), sbuf))
            sk = self.dist_levels[self.k][i]
            bk = _bs(sk)
            b["bk"] = ops.zeros(max(self.counts) * bk)
            b["bglob"] = ops.zeros(int(self.offs[-1]) * bk)
            b["xglob"] = ops.zeros(int(self.offs[-1]) * bk)
            b["nk"] = sk.n * bk
            b["bsk"] = bk
            if self.fold:
                # level k in the [owned | ghost] layout of this rank, picked from the replicated tail solution
                gmap = self.level_k_map(i)
                b["kmap"] = ops.index(gmap)
                b["xk_ext"] = ops.zeros(gmap.size)
            self.buf.append(b)

    def _halo(self, l, key):
        sends, recvs = [], []
        for i, ops in enumerate(self.ops):
            s, b = self.dist_levels[l][i], self.buf[i]
            vec = b[key][l]
            idx, sbuf = b["sidx"][l]
            if sbuf.numel():
                ops.gather(vec, idx, sbuf)
            sends.append(b["send"][l])
            recvs.append({q: vec[(s.n + a) * _bs(s):(s.n + e) * _bs(s)] for q, (a, e) in s.recv_seg.items()})
        self.comm.halo(sends, recvs)

    def rhs_buffer(self, i=0):
        """owned part of the level-0 right-hand-side buffer of local rank i: fill THIS tensor and pass it to Mult to
        save the copy of b into the [owned | ghost] layout (Jacobi path)"""
        if self._dev is not None:
            return self._dev.rhs_buffer(i)
        return self.buf[i]["bext"][0][:self.dist_levels[0][i].n]

    def Mult(self, bs, xs, b_status=1):
        """bs[i], xs[i]: owned level-0 vectors of local rank i (tensors of the backend's kind).  Collective: every rank of
        the communicator calls it (AMGMatrix::Mult, amg_matrix.cpp:160-307).  b_status 0 (device path only): bs[i] has
        [owned | ghost] entries, the ghost entries are added to their owners first (DISTRIBUTED vector)"""
        if self._dev is not None:
            return self._dev.Mult(bs, xs, b_status)
        if self.sm_type in ("gs", "hgs", "bgs"):
            return self._mult_gs(bs, xs)
        if self.fold:
            return self._mult_folded(bs, xs)
        k = self.k
        nown = lambda l, i: self.dist_levels[l][i].n * _bs(self.dist_levels[l][i])        # owned scalar entries
        for l in range(k):
            for i, ops in enumerate(self.ops):
                s, b = self.dist_levels[l][i], self.buf[i]
                if l == 0 and bs[i].data_ptr() != b["bext"][0].data_ptr():
                    b["bext"][0][:nown(0, i)].copy_(bs[i])
            self._halo(l, "bext")
            for i, ops in enumerate(self.ops):
                s, b = self.dist_levels[l][i], self.buf[i]
                xl = xs[i] if l == 0 else b["x"][l]
                ops.jacobi_pre(l, b["bext"][l], xl, b["r"][l])
                nxt = b["bext"][l + 1][:nown(l + 1, i)] if l + 1 < k else b["bk"][:b["nk"]]
                ops.restrict(l, b["r"][l], nxt)
        # replicated tail: all-gather the level-k right-hand side, every rank runs the same serial cycle
        bk = self.buf[0]["bsk"]
        self.comm.allgather_tensor([b["bk"] for b in self.buf], [b["bglob"] for b in self.buf], [c * bk for c in self.counts])
        for i, ops in enumerate(self.ops):
            b = self.buf[i]
            ops.tail_apply(b["bglob"], b["xglob"])
        for l in range(k - 1, -1, -1):
            for i, ops in enumerate(self.ops):
                s, b = self.dist_levels[l][i], self.buf[i]
                r = self.dist_levels[l][i].rank
                xc = b["x"][l + 1] if l + 1 < k else b["xglob"][int(self.offs[r]) * bk:int(self.offs[r]) * bk + b["nk"]]
                xl = xs[i] if l == 0 else b["x"][l]
                ops.prolong(l, xl, xc, b["text"][l][:nown(l, i)])
            self._halo(l, "text")
            for i, ops in enumerate(self.ops):
                s, b = self.dist_levels[l][i], self.buf[i]
                xl = xs[i] if l == 0 else b["x"][l]
                ops.jacobi_post(l, b["text"][l], b["bext"][l][:nown(l, i)], xl)
        return xs

    def _mult_folded(self, bs, xs):
        """Jacobi V(1,1) in the form the single-GPU cycle runs: down = fused pre-smoothing + restriction
        writing z = S(S0 b); up = x = z + Q x_c.  Exchanges: b before every down stage, x of the levels 1..k-1 after their
        up stage (level k comes replicated from the tail) -- 2k - 1 instead of 2k."""
        k = self.k
        for l in range(k):
            for i, ops in enumerate(self.ops):
                s, b = self.dist_levels[l][i], self.buf[i]
                if l == 0 and bs[i].data_ptr() != b["bext"][0].data_ptr():
                    b["bext"][0][:s.n].copy_(bs[i])
            self._halo(l, "bext")
            for i, ops in enumerate(self.ops):
                s, b = self.dist_levels[l][i], self.buf[i]
                xl = xs[i] if l == 0 else b["xext"][l][:s.n]
                nxt = b["bext"][l + 1][:self.dist_levels[l + 1][i].n] if l + 1 < k else b["bk"][:b["nk"]]
                ops.cycle_down(l, b["bext"][l], xl, nxt)
        self.comm.allgather_tensor([b["bk"] for b in self.buf], [b["bglob"] for b in self.buf], self.counts)
        for i, ops in enumerate(self.ops):
            b = self.buf[i]
            ops.tail_apply(b["bglob"], b["xglob"])
            ops.gather(b["xglob"], b["kmap"], b["xk_ext"])
        for l in range(k - 1, -1, -1):
            for i, ops in enumerate(self.ops):
                s, b = self.dist_levels[l][i], self.buf[i]
                xl = xs[i] if l == 0 else b["xext"][l][:s.n]
                ops.cycle_up(l, xl, b["xext"][l + 1] if l + 1 < k else b["xk_ext"])
            if l > 0:
                self._halo(l, "xext")
        return xs

    def _mult_gs(self, bs, xs):
        """V(1,1) with the hybrid Gauss-Seidel smoother on the rank-partitioned levels:
        pre  : x = 0; forward sweep on the owned rows (all off-rank values are 0); halo(x); r = b - A x; restrict
        post : x += P x_c; halo(x); backward sweep with the off-rank values frozen (reference stages: gssmoother.cpp:709-861)"""
        k = self.k
        for l in range(k):
            for i, ops in enumerate(self.ops):
                s, b = self.dist_levels[l][i], self.buf[i]
                bl = bs[i] if l == 0 else b["b"][l]
                b["xext"][l].zero_()
                ops.gs_sweep(l, 0, b["xext"][l], bl, b["r"][l])
            self._halo(l, "xext")
            for i, ops in enumerate(self.ops):
                s, b = self.dist_levels[l][i], self.buf[i]
                bl = bs[i] if l == 0 else b["b"][l]
                ops.residual(l, b["xext"][l], bl, b["r"][l])
                nxt = b["b"][l + 1] if l + 1 < k else b["bk"][:b["nk"]]
                ops.restrict(l, b["r"][l], nxt)
        self.comm.allgather_tensor([b["bk"] for b in self.buf], [b["bglob"] for b in self.buf], [c * self.buf[0]["bsk"] for c in self.counts])
        for i, ops in enumerate(self.ops):
            b = self.buf[i]
            ops.tail_apply(b["bglob"], b["xglob"])
        for l in range(k - 1, -1, -1):
            for i, ops in enumerate(self.ops):
                s, b = self.dist_levels[l][i], self.buf[i]
                r = s.rank
                sc = self.dist_levels[l + 1][i] if l + 1 < k else None
                xc = (b["xext"][l + 1][:sc.n * _bs(sc)] if l + 1 < k else
                      b["xglob"][int(self.offs[r]) * b["bsk"]:int(self.offs[r]) * b["bsk"] + b["nk"]])
                xo = b["xext"][l][:s.n * _bs(s)]
                ops.prolong(l, xo, xc, xo)
            self._halo(l, "xext")
            for i, ops in enumerate(self.ops):
                s, b = self.dist_levels[l][i], self.buf[i]
                bl = bs[i] if l == 0 else b["b"][l]
                ops.gs_sweep(l, 1, b["xext"][l], bl, b["r"][l])
                if l == 0:
                    xs[i].copy_(b["xext"][0][:s.n * _bs(s)])
        return xs

    # ---- the same hierarchy as ONE global serial hierarchy (for the oracle / tests) -----------------------------
    def global_levels(self):
        """assemble the global level matrices / prolongations from all ranks (loopback or gathered) as Level objects"""
        comm = self.comm
        out = []
        for l in range(self.k):
            lv = self.dist_levels[l]
            cnt = comm.allgather([s.n for s in lv])[0]
            off = np.concatenate([[0], np.cumsum(cnt)])
            nxt = self.dist_levels[l + 1]
            cntc = comm.allgather([s.n for s in nxt])[0]
            offc = np.concatenate([[0], np.cumsum(cntc)])
            pa, pp, pf, pd = [], [], [], []
            bf = _bs(lv[0])
            bc = int(getattr(lv[0], "bs_c", bf))
            for s in lv:
                gmapv = np.concatenate([off[s.rank] + np.arange(s.n), off[s.ghost_owner] + s.ghost_rindex]).astype(np.int64)
                A = sp.csr_matrix(s.A)
                cv, cc = np.divmod(A.indices, bf)
                pa.append((s.rank, np.diff(A.indptr), gmapv[cv] * bf + cc, A.data))
                P = sp.csr_matrix(s.P)
                pp.append((s.rank, np.diff(P.indptr), offc[s.rank] * bc + P.indices, P.data))
                pf.append((s.rank, s.free))
                pd.append((s.rank, s.dinv_ext[:s.n * bf * bf]))
            ga = sorted(comm.allgather(pa)[0], key=lambda t: t[0])
            gp = sorted(comm.allgather(pp)[0], key=lambda t: t[0])
            gf = sorted(comm.allgather(pf)[0], key=lambda t: t[0])
            gd = sorted(comm.allgather(pd)[0], key=lambda t: t[0])
            n, nc = int(off[-1]), int(offc[-1])
            A = sp.csr_matrix((np.concatenate([t[3] for t in ga]), np.concatenate([t[2] for t in ga]),
                               np.concatenate([[0]] + [t[1] for t in ga]).cumsum()), shape=(n * bf, n * bf))
            P = sp.csr_matrix((np.concatenate([t[3] for t in gp]), np.concatenate([t[2] for t in gp]),
                               np.concatenate([[0]] + [t[1] for t in gp]).cumsum()), shape=(n * bf, nc * bc))
            A.sort_indices()
            P.sort_indices()
            PT = sp.csr_matrix(P.T)
            PT.sort_indices()
            free = np.concatenate([t[1] for t in gf]).astype(np.uint8)
            L = Level(A=_mat(A, bf), P=_mat(P, bf, bc), PT=_mat(PT, bc, bf), free=free, dinv=np.concatenate([t[1] for t in gd]),
                      coords=None, color=np.full(n, -1, dtype=np.int32), n_colors=0, agg=None)
            if self.sm_type == "gs":
                # hybrid GS as ONE serial smoother: every rank is a block, its rows are visited in its colour-major order
                pg = [(s.rank, s.dinv_gs_ext[:s.n * bf * bf], s.color) for s in lv]
                gg = sorted(comm.allgather(pg)[0], key=lambda t: t[0])
                L.dinv = np.concatenate([t[1] for t in gg])
                order, block = [], []
                for t in gg:
                    rows = np.nonzero(t[2] >= 0)[0]
                    order.append(off[t[0]] + rows[np.argsort(t[2][rows], kind="stable")])
                    block.append(np.full(t[2].size, t[0], dtype=np.int32))
                L.gs_order = np.concatenate(order).astype(np.int32)
                L.gs_block = np.concatenate(block)
            if self.sm_type == "hgs":
                pg = [(s.rank, s.dinv_gs_ext[:s.n * bf * bf], s.gs_order, s.gs_blockid) for s in lv]
                gg = sorted(comm.allgather(pg)[0], key=lambda t: t[0])
                L.dinv = np.concatenate([t[1] for t in gg])
                order, block, boff = [], [], 0
                for t in gg:
                    order.append(off[t[0]] + t[2])
                    block.append(boff + t[3])
                    boff += int(t[3].max()) + 1 if t[3].size else 0
                L.gs_order = np.concatenate(order).astype(np.int32)
                L.gs_block = np.concatenate(block).astype(np.int32)
            if self.sm_type == "bgs":
                # hybrid block GS as ONE serial smoother: blocks of all ranks (global row ids), visited rank by rank and
                # colour-major inside a rank; rows of another rank are read at their sweep-start values (gs_block)
                from .hierarchy import BGSData
                pg = [(s.rank, s.n, s.bgs.block_ptr, s.bgs.block_rows, s.bgs.dinv_ptr, s.bgs.dinv, s.bgs.color) for s in lv]
                gg = sorted(comm.allgather(pg)[0], key=lambda t: t[0])
                bptr, brow, dptr, dval, order, col, block = [np.zeros(1, dtype=np.int64)], [], [np.zeros(1, dtype=np.int64)], [], [], [], []
                nb = 0
                for r, nloc, bp, br, dp, dv, cc in gg:
                    bptr.append(bptr[-1][-1] + np.asarray(bp[1:], dtype=np.int64))
                    brow.append(off[r] + np.asarray(br, dtype=np.int64))
                    dptr.append(dptr[-1][-1] + np.asarray(dp[1:], dtype=np.int64))
                    dval.append(np.asarray(dv)[:int(dp[-1])])
                    order.append(nb + np.argsort(np.asarray(cc), kind="stable"))
                    col.append(np.asarray(cc))
                    block.append(np.full(nloc, r, dtype=np.int32))
                    nb += len(cc)
                L.bgs = BGSData(nb, np.concatenate(bptr).astype(np.int32), np.concatenate(brow).astype(np.int32),
                                np.concatenate(dptr).astype(np.int64), np.concatenate(dval) if dval else np.zeros(1),
                                np.concatenate(col).astype(np.int32), int(max(c.max() for c in col) + 1) if nb else 0,
                                order=np.concatenate(order).astype(np.int32))
                L.gs_block = np.concatenate(block)
            out.append(L)
        tail = []
        for L in self.tail_hier.levels:
            if getattr(L, "hgs_pre", None) is not None:
                from copy import copy
                L2 = copy(L)
                L2.dinv = np.ascontiguousarray(L.hgs_dinv[:L.A.n_rows * L.A.br * L.A.br])
                tail.append(L2)
            else:
                tail.append(L)
        return out + tail


def _gs_stages(comm, states, min_rows):
    """Stages of the hybrid Gauss-Seidel sweep as colour ranges (reference: LOC_1 = rows [0, split), EX = rows shared with
    other ranks, LOC_2 = rows [split, N), split_ind = N/2, gssmoother.cpp:664-678, 721-782): colours are re-indexed so that
    the first half of the interior rows comes first, then the boundary rows, then the second half of the interior rows.  The
    exchange of x is hidden behind a local stage in both sweep directions.  Small levels keep one stage (three times the
    colours would be three times the dependent launches)."""
    big = min(min(x) for x in comm.allgather([s.n for s in states])) >= min_rows
    for s in states:
        nc = int(s.n_colors)
        if not big or s.n_interior < 2:
            s.gs_stage = np.array([0, 0, nc, nc], dtype=np.int32)
            continue
        half = s.n_interior // 2
        grp = np.ones(s.n, dtype=np.int64)
        grp[:half] = 0
        grp[half:s.n_interior] = 2
        col = np.asarray(s.color, dtype=np.int64)
        act = col >= 0
        key = grp[act] * (nc + 1) + col[act]
        uniq, inv = np.unique(key, return_inverse=True)
        newc = np.full(s.n, -1, dtype=np.int32)
        newc[act] = inv.astype(np.int32)
        g_of = uniq // (nc + 1)
        s1, s2 = int((g_of == 0).sum()), int((g_of <= 1).sum())
        s.color, s.n_colors = newc, int(uniq.size)
        s.gs_stage = np.array([0, s1, s2, int(uniq.size)], dtype=np.int32)


class _CudaBuffer:
    """device memory owned by the native library, exposed through __cuda_array_interface__ (torch.as_tensor)"""

    def __init__(self, addr, n, owner):
        self.__cuda_array_interface__ = {"shape": (int(n),), "typestr": "<f8", "data": (int(addr), False), "version": 2, "strides": None}
        self._owner = owner


class _DeviceDist:
    """Rank-partitioned hierarchy on the GPU(s) behind the C ABI (include/amgx.h: amgx_comm_*, amgx_dist_*).
    LoopbackComm -> AMGX_COMM_LOCAL (all ranks in this process on one GPU), TorchComm -> AMGX_COMM_RCCL (one rank per
    process; torch.distributed only carries the 128-byte RCCL id and the host-side setup messages)."""

    def __init__(self, amg, device):
        import torch
        from .device import DeviceAMGMatrix, hierarchy_desc
        lib = _lib.hip()
        self._lib, self.amg, self.device = lib, amg, int(device)
        comm = amg.comm
        self._comm = C.c_void_p()
        if isinstance(comm, LoopbackComm):
            rc = lib.amgx_comm_create(_lib.AMGX_COMM_LOCAL, comm.size, 0, None, self.device, C.byref(self._comm))
        else:
            uid = C.create_string_buffer(_lib.AMGX_UNIQUE_ID_BYTES)
            if comm.rank == 0 and lib.amgx_comm_unique_id(uid) != 0:
                raise NgsAMGError(lib.amgx_comm_last_error(None).decode())
            ids = comm.allgather([uid.raw])[0]
            torch.cuda.set_device(self.device)
            rc = lib.amgx_comm_create(_lib.AMGX_COMM_RCCL, comm.size, comm.rank, ids[0], self.device, C.byref(self._comm))
        if rc != 0:
            raise NgsAMGError(lib.amgx_comm_last_error(None).decode())
        k = amg.k
        sm = amg.sm_type
        self._dists, self.ops, self._keep = [], [], []

        class _Ops:
            pass
        for i, top in enumerate(amg.tops):
            types = [sm] * (top.n_levels - 1) + ["jacobi"]
            stp, sym, cyc = getattr(amg, "sm_steps", 1), getattr(amg, "sm_symm", False), getattr(amg, "mg_cycle", "V")
            cheb = {}
            if sm == "cheby":
                lam = amg.cheb_lambda_max
                if isinstance(lam, (list, tuple, np.ndarray)):
                    if len(lam) != k:
                        raise NgsAMGError(f"cheb_lambda_max list must have one entry per rank-partitioned level ({k})")
                    lam = list(lam)
                else:
                    lam = [lam] * k
                cheb = dict(cheb_degree=amg.cheb_degree, cheb_ratio=amg.cheb_ratio)
                tcheb = dict(cheb, cheb_lambda_max=lam + [None])
            else:
                tcheb = {}
            tdesc, tkeep, _ = hierarchy_desc(top, sm_type=types, omega=amg.omega, clev="none", device=self.device, use_graph=False,
                                             sm_steps=stp, sm_symm=sym, mg_cycle=cyc, **tcheb)
            ldesc, lkeep, _ = hierarchy_desc(amg.tail_hier, sm_type=sm, omega=amg.omega, device=self.device, sm_steps=stp, sm_symm=sym, mg_cycle=cyc,
                                             **cheb)
            halos = (_lib.amgx_halo_desc * k)()
            keep = [tkeep, lkeep, halos]
            for l in range(k):
                s = amg.dist_levels[l][i]
                peers = sorted(set(s.send) | set(s.recv_seg))
                send_ptr = np.zeros(len(peers) + 1, dtype=np.int64)
                recv_ptr = np.zeros(len(peers) + 1, dtype=np.int64)
                idx = []
                pos = 0
                for j, q in enumerate(peers):
                    v = s.send.get(q, np.empty(0, dtype=np.int64))
                    idx.append(np.asarray(v, dtype=np.int32))
                    send_ptr[j + 1] = send_ptr[j] + v.size
                    a, b = s.recv_seg.get(q, (pos, pos))
                    if a != pos:
                        raise NgsAMGError("halo tables: ghost segments are not in peer order")
                    pos = b
                    recv_ptr[j + 1] = b
                pr = np.asarray(peers, dtype=np.int32)
                si = np.ascontiguousarray(np.concatenate(idx) if idx else np.empty(0, dtype=np.int32), dtype=np.int32)
                h = halos[l]
                h.n_peers = len(peers)
                h.peer_rank, h.send_ptr, h.send_idx, h.recv_ptr = _lib.ptr(pr, C.c_int32), _lib.ptr(send_ptr, C.c_int64), _lib.ptr(si, C.c_int32), _lib.ptr(recv_ptr, C.c_int64)
                h.n_interior = int(getattr(s, "n_interior", 0))
                keep += [pr, send_ptr, si, recv_ptr]
            counts = np.asarray(amg.counts, dtype=np.int64)
            kmap = np.ascontiguousarray(amg.level_k_map(i), dtype=np.int64)
            d = _lib.amgx_dist_desc()
            d.top, d.tail, d.halo = tdesc, ldesc, halos
            d.counts, d.kmap, d.kmap_len = _lib.ptr(counts, C.c_int64), _lib.ptr(kmap, C.c_int64), kmap.size
            d.rank = int(amg.dist_levels[0][i].rank)
            d.fold = int(amg.fold)
            d.cheby = int(sm == "cheby")
            if sm == "gs":
                st = np.ascontiguousarray(np.concatenate([amg.dist_levels[l][i].gs_stage for l in range(k)]), dtype=np.int32)
                d.gs_stage = _lib.ptr(st, C.c_int32)
                keep.append(st)
            keep += [counts, kmap]
            hd = C.c_void_p()
            rc = lib.amgx_dist_create(self._comm, C.byref(d), C.byref(hd))
            msg = lib.amgx_comm_last_error(self._comm).decode() if rc != 0 else ""
            # amgx_dist_create is not collective: a failure on ONE rank (e.g. a level its kernels cannot take) must stop
            # every rank here, before the first collective of amgx_dist_apply would leave the others waiting in RCCL
            if not isinstance(comm, LoopbackComm):
                msgs = comm.allgather([msg])[0]
                bad = [(r, m) for r, m in enumerate(msgs) if m]
                if bad:
                    raise NgsAMGError("amgx_dist_create failed on rank(s) " + "; ".join(f"{r}: {m}" for r, m in bad))
            elif rc != 0:
                raise NgsAMGError(msg)
            self._dists.append(hd)
            self._keep.append(keep)
            ht, hl = C.c_void_p(), C.c_void_p()
            lib.amgx_dist_handles(hd, C.byref(ht), C.byref(hl))
            o = _Ops()
            o.top, o.tail = DeviceAMGMatrix.view(ht, top), DeviceAMGMatrix.view(hl, amg.tail_hier)
            self.ops.append(o)
        self._keep = []           # the native side copied everything
        # collective lambda_max estimate of the rank-partitioned Chebyshev levels: every rank exists now (a no-op otherwise)
        self._ck(lib.amgx_dist_cheb_estimate(self._comm))
        self._stream = None
        self._rhs = {}

    def __del__(self):
        c = getattr(self, "_comm", None)
        if c:
            for o in getattr(self, "ops", []):
                o.top._h = o.tail._h = None
            self._lib.amgx_comm_destroy(c)
            self._comm = None

    def _ck(self, rc):
        if rc != 0:
            raise NgsAMGError(self._lib.amgx_comm_last_error(self._comm).decode())

    def rhs_buffer(self, i=0):
        import torch
        if i not in self._rhs:
            p, n, ne = C.c_void_p(), C.c_int64(), C.c_int64()
            self._lib.amgx_dist_rhs_buffer(self._dists[i], C.byref(p), C.byref(n), C.byref(ne))
            t = torch.as_tensor(_CudaBuffer(p.value, ne.value, self), device=torch.device("cuda", self.device))
            self._rhs[i] = (t, n.value)
        t, n = self._rhs[i]
        return t[:n]

    def rhs_buffer_ext(self, i=0):
        self.rhs_buffer(i)
        return self._rhs[i][0]

    def _bind_stream(self):
        """the communicator works on torch's current stream.  On the legacy default stream (handle 0) it keeps its own
        non-blocking stream (a null stream cannot be captured into the cycle's graph), which torch's default stream does not
        order with: what the caller enqueued there so far (allocations, fills, the right-hand side) is waited for here."""
        import torch
        cur = torch.cuda.current_stream()
        st = int(cur.cuda_stream)
        if st == 0:
            cur.synchronize()
        if st != self._stream:
            self._ck(self._lib.amgx_comm_set_stream(self._comm, C.c_void_p(st)))
            self._stream = st

    def Mult(self, bs, xs, b_status=1):
        import torch
        self._bind_stream()
        n = len(self._dists)
        if len(bs) != n or len(xs) != n:
            raise NgsAMGError("Mult: one b and one x per local rank")
        for i, (b, x) in enumerate(zip(bs, xs)):
            s = self.amg.dist_levels[0][i]
            nb = (s.n if b_status else s.n + s.ghost_owner.size) * _bs(s)
            for v, m, nm in ((b, nb, "b"), (x, s.n * _bs(s), "x")):
                if not (v.is_cuda and v.dtype == torch.float64 and v.is_contiguous() and v.numel() == m):
                    raise NgsAMGError(f"{nm}[{i}]: need a contiguous float64 CUDA tensor with {m} entries")
        pb = (C.c_void_p * n)(*[b.data_ptr() for b in bs])
        px = (C.c_void_p * n)(*[x.data_ptr() for x in xs])
        self._ck(self._lib.amgx_dist_apply(self._comm, pb, px, int(b_status), _lib.AMGX_DEVICE_PTR))
        return xs

    def time_kernel(self, level, op=8, reps=20):
        """amgx_dist_time_kernel (collective): average ms of the level's dominant kernel inside the running cycle"""
        self._bind_stream()
        ms = C.c_double()
        self._ck(self._lib.amgx_dist_time_kernel(self._comm, int(level), int(op), int(reps), C.byref(ms)))
        return ms.value

    def n_exchanges(self):
        ne = C.c_int64()
        self._ck(self._lib.amgx_comm_info(self._comm, None, None, None, C.byref(ne)))
        return ne.value

    def pcg(self, bs, xs, tol=1e-8, maxsteps=200, use_pre=True, single_reduction=False):
        """amgx_dist_pcg: collective PCG with the rank-partitioned cycle as preconditioner; xs hold the initial guess and
        receive the solution.  Returns (iterations, err_0 .. err_iterations).  single_reduction: one all-reduce of two scalars per
        iteration (AMGX_PCG_SINGLE_REDUCTION) instead of two of one."""
        import torch
        self._bind_stream()
        n = len(self._dists)
        for i, (b, x) in enumerate(zip(bs, xs)):
            m = self.amg.dist_levels[0][i].n * _bs(self.amg.dist_levels[0][i])
            for v, nm in ((b, "b"), (x, "x")):
                if not (v.is_cuda and v.dtype == torch.float64 and v.is_contiguous() and v.numel() == m):
                    raise NgsAMGError(f"{nm}[{i}]: need a contiguous float64 CUDA tensor with {m} entries")
        pb = (C.c_void_p * n)(*[b.data_ptr() for b in bs])
        px = (C.c_void_p * n)(*[x.data_ptr() for x in xs])
        errs = np.zeros(int(maxsteps) + 1)
        it = C.c_int32()
        self._ck(self._lib.amgx_dist_pcg(self._comm, pb, px, float(tol), int(maxsteps), int(bool(use_pre)),
                                         _lib.AMGX_DEVICE_PTR | (_lib.AMGX_PCG_SINGLE_REDUCTION if single_reduction else 0),
                                         _lib.ptr(errs, C.c_double), C.byref(it)))
        return it.value, errs[:it.value + 1]

    def gmres(self, bs, xs, tol=1e-8, maxsteps=200, restart=30, use_pre=True):
        """amgx_dist_gmres: collective restarted GMRES with the rank-partitioned cycle as (left) preconditioner; xs hold the initial
        guess and receive the solution.  Returns (iterations, err_0 .. err_iterations)."""
        import torch
        self._bind_stream()
        n = len(self._dists)
        for i, (b, x) in enumerate(zip(bs, xs)):
            m = self.amg.dist_levels[0][i].n * _bs(self.amg.dist_levels[0][i])
            for v, nm in ((b, "b"), (x, "x")):
                if not (v.is_cuda and v.dtype == torch.float64 and v.is_contiguous() and v.numel() == m):
                    raise NgsAMGError(f"{nm}[{i}]: need a contiguous float64 CUDA tensor with {m} entries")
        pb = (C.c_void_p * n)(*[b.data_ptr() for b in bs])
        px = (C.c_void_p * n)(*[x.data_ptr() for x in xs])
        errs = np.zeros(int(maxsteps) + 1)
        it = C.c_int32()
        self._ck(self._lib.amgx_dist_gmres(self._comm, pb, px, float(tol), int(maxsteps), int(restart), int(bool(use_pre)), _lib.AMGX_DEVICE_PTR,
                                           _lib.ptr(errs, C.c_double), C.byref(it)))
        return it.value, errs[:it.value + 1]

    def graph_info(self):
        """whole-cycle graph of amgx_dist_apply: enabled?, captured cycles, applications served by a graph launch, note"""
        en, ng, nr = C.c_int32(), C.c_int64(), C.c_int64()
        self._ck(self._lib.amgx_comm_graph_info(self._comm, C.byref(en), C.byref(ng), C.byref(nr)))
        return {"enabled": bool(en.value), "graphs": ng.value, "replays": nr.value,
                "note": (self._lib.amgx_comm_graph_note(self._comm) or b"").decode()}

    def order_info(self):
        """how directly launched work on the two streams is ordered: "events" or "flags" (amgx_comm_order_info)"""
        ev = C.c_int32()
        self._ck(self._lib.amgx_comm_order_info(self._comm, C.byref(ev)))
        return "events" if ev.value else "flags"

    def synchronize(self):
        self._ck(self._lib.amgx_comm_synchronize(self._comm))
