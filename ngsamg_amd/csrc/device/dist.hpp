// Rank-partitioned levels: communicator, halo exchange and the collective V-cycle (included by amgx.hip).
//
// Reference counterparts (not its code):
//   Comm        <-> the MPI communicator of the ParallelDofs                     (src/base/linalg/dcc_map.hpp:20-90)
//   HaloTable   <-> DCCMap tables m_ex_dofs / g_ex_dofs + buffers                (dcc_map.cpp:17-65, 480-543)
//   exchange()  <-> StartCO2CU / ApplyCO2CU (owner -> ghost, overwrite) and StartDIS2CO / ApplyDIS2CO (ghost -> owner,
//                   add)                                                         (dcc_map.cpp:76-178, 249-302)
//   Dist::apply <-> AMGMatrix::SmoothV called collectively by every rank        (src/base/solve/amg_matrix.cpp:160-307)
//                   with HybridSmoother stages around the exchanges              (hybrid_base_smoother.cpp:501-574)
//
// MI355X design: one process per GPU; a rank stores the rows of the vertices it OWNS with columns [owned | ghost]
// (DESIGN.md 5.4), ghosts grouped by owner, so a peer's message lands contiguously (no unpack kernel in the owner ->
// ghost direction).  Owned rows are ordered [interior | boundary]: kernels on the interior rows run on the compute stream
// while pack kernel + ncclSend/ncclRecv run on the communication stream; the boundary part waits for the exchange event.
// Nothing here synchronises the host: one application is one burst of asynchronous launches.
#pragma once
#include <dlfcn.h>
#include <rccl/rccl.h>

namespace amgx {

// ---------------------------------------------------------------------------------------------------
// RCCL entry points, resolved at run time: a process that already holds a copy of librccl (torch ships one)
// must not get a second one through a link-time dependency.
struct Rccl {
  void* lib = nullptr;
  ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*Send)(const void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*Recv)(void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*GroupStart)() = nullptr;
  ncclResult_t (*GroupEnd)() = nullptr;
  const char* (*GetErrorString)(ncclResult_t) = nullptr;

  static Rccl& get() {
    static Rccl r;
    if (r.lib) return r;
    const char* names[] = {std::getenv("NGSAMG_RCCL_LIB"), "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    void* h = dlopen("librccl.so.1", RTLD_NOW | RTLD_NOLOAD);       // the copy this process already uses, if any
    for (int i = 0; i < 4 && !h; ++i) if (names[i] && *names[i]) h = dlopen(names[i], RTLD_NOW | RTLD_GLOBAL);
    if (!h) throw Err(std::string("RCCL not found (librccl.so.1): ") + (dlerror() ? dlerror() : "?") + "; set NGSAMG_RCCL_LIB");
    auto sym = [&](const char* n) { void* p = dlsym(h, n); if (!p) throw Err(std::string("librccl: missing symbol ") + n); return p; };
    r.GetUniqueId = (decltype(r.GetUniqueId))sym("ncclGetUniqueId");
    r.CommInitRank = (decltype(r.CommInitRank))sym("ncclCommInitRank");
    r.CommDestroy = (decltype(r.CommDestroy))sym("ncclCommDestroy");
    r.Send = (decltype(r.Send))sym("ncclSend");
    r.Recv = (decltype(r.Recv))sym("ncclRecv");
    r.AllGather = (decltype(r.AllGather))sym("ncclAllGather");
    r.AllReduce = (decltype(r.AllReduce))sym("ncclAllReduce");
    r.GroupStart = (decltype(r.GroupStart))sym("ncclGroupStart");
    r.GroupEnd = (decltype(r.GroupEnd))sym("ncclGroupEnd");
    r.GetErrorString = (decltype(r.GetErrorString))sym("ncclGetErrorString");
    r.lib = h;
    return r;
  }
};

#define NCCLCHK(call)                                                                                              \
  do {                                                                                                             \
    ncclResult_t r_ = (call);                                                                                      \
    if (r_ != ncclSuccess)                                                                                         \
      throw ::amgx::Err(std::string(#call) + " failed: " + ::amgx::Rccl::get().GetErrorString(r_) + " (" __FILE__ ":" + std::to_string(__LINE__) + ")"); \
  } while (0)

// ---------------------------------------------------------------------------------------------------
// device-to-device copy as a kernel of our own (see vec_copy_kernel)
static inline void dev_copy(double* dst, const double* src, int64_t n, hipStream_t st) {
  if (n <= 0 || dst == src) return;
  launch(vec_copy_kernel, (unsigned)(((n + 1) / 2 + BLOCK - 1) / BLOCK), BLOCK, 0, st, n, src, dst);
}

struct HaloTable {                       // one level of one rank
  int bs = 1;
  int64_t n = 0, n_ghost = 0, n_int = 0; // owned block rows, ghost block rows, interior rows (no ghost column)
  std::vector<int> peers;                // ascending ranks
  std::vector<int64_t> send_ptr, recv_ptr;   // [n_peers + 1] in block rows
  DevBuf<int32_t> send_idx;              // owned block rows packed per peer (m_ex_dofs)
  DevBuf<double> sendbuf;                // pack target / receive buffer of the add direction
  int64_t n_send() const { return send_ptr.empty() ? 0 : send_ptr.back(); }

  void build(const amgx_halo_desc& d, int64_t n_own, int64_t n_cols, int bsz, int nranks, int self) {
    bs = bsz; n = n_own; n_ghost = n_cols - n_own;
    if (d.n_peers < 0 || (d.n_peers > 0 && (!d.peer_rank || !d.send_ptr || !d.recv_ptr))) throw Err("halo table: missing arrays");
    n_int = d.n_interior;
    if (n_int < 0 || n_int > n) throw Err("halo table: n_interior out of range");
    peers.assign(d.peer_rank, d.peer_rank + d.n_peers);
    send_ptr.assign(d.n_peers + 1, 0); recv_ptr.assign(d.n_peers + 1, 0);
    for (int k = 0; k <= d.n_peers; ++k) { send_ptr[k] = d.send_ptr[k]; recv_ptr[k] = d.recv_ptr[k]; }
    for (int k = 0; k < d.n_peers; ++k) {
      if (peers[k] < 0 || peers[k] >= nranks || (k && peers[k] <= peers[k - 1])) throw Err("halo table: peers must be ascending valid ranks");
      if (peers[k] == self && nranks > 1) throw Err("halo table: a rank cannot be its own peer");
      if (send_ptr[k + 1] < send_ptr[k] || recv_ptr[k + 1] < recv_ptr[k]) throw Err("halo table: pointers must be monotone");
    }
    if (send_ptr[0] != 0 || recv_ptr[0] != 0) throw Err("halo table: pointers must start at 0");
    if (recv_ptr.back() != n_ghost) throw Err("halo table: the receive segments must cover the ghost block exactly");
    const int64_t ns = n_send();
    if (ns >= I32_MAX) throw Err("halo table: too many send entries");
    if (ns > 0 && !d.send_idx) throw Err("halo table: send_idx missing");
    for (int64_t i = 0; i < ns; ++i) if (d.send_idx[i] < 0 || d.send_idx[i] >= n) throw Err("halo table: send index out of the owned range");
    // the boundary-row contract behind the overlap: a row that READS a ghost must not be interior -- a property of the matrix,
    // checked where the matrix is known (dist_create).  A SENT row may be interior for the Jacobi stages (what is sent is
    // complete before the exchange starts); the Gauss-Seidel stages need more, also checked in dist_create
    if (ns) send_idx.upload(d.send_idx, (size_t)ns);
    sendbuf.alloc((size_t)std::max<int64_t>(1, std::max<int64_t>(ns, 1) * bs));
  }
  int peer_pos(int q) const { for (size_t k = 0; k < peers.size(); ++k) if (peers[k] == q) return (int)k; return -1; }
};

struct Dist;
// The driver of the collective cycle (DistCycle), resolved once by dist_create.  The first four and CHEBY are the specialised
// V(1,1) stage sequences; STEPWISE serves sm_steps > 1 / sm_symm on a rank-partitioned level and the W-cycle.
enum class DistPath {
  JACOBI_FOLDED,       // Jacobi, post-smoothing folded into the prolongation
  JACOBI_LITERAL,      // Jacobi in the literal stage order
  GS_BLOCK_HYBRID,     // Gauss-Seidel levels in the block-hybrid form (gs_block_rows)
  GS_STAGED,           // multicolour / aggregate-block Gauss-Seidel in colour stages
  STEPWISE,            // one exchange and one launch per smoothing step
  CHEBY,               // Chebyshev: the schedule of cheb_schedule.hpp, every product step behind the exchange of its iterate
};
}  // namespace amgx
struct amgx_dist_t { amgx::Dist* d; };
namespace amgx {

struct Comm {
  int kind = AMGX_COMM_LOCAL, nranks = 1, rank = 0, device = 0;
  ncclComm_t nccl = nullptr;
  hipStream_t own_compute = nullptr, compute = nullptr, comm_stream = nullptr;
  static constexpr int NEV = 8;
  hipEvent_t ev_ready[NEV], ev_done[NEV];
  int ev_next = 0;
  std::vector<Dist*> members;            // local ranks in creation order (RCCL: exactly one)
  // C-ABI wrappers handed out for this communicator's objects (amgx_dist_create, amgx_dist_handles): owned here, so that
  // amgx_comm_destroy can null them -- a call through a stale wrapper then returns an error instead of touching freed memory
  std::vector<amgx_dist_t*> dist_wrappers;
  std::vector<amgx_handle_t*> handle_views;
  std::string err;
  int64_t n_exchanges = 0;               // statistics: halo exchanges started
  bool cheb_estimate_done = false;       // the collective lambda_max estimate has run (dist_cheb_estimate: once, before any capture)
  // Cross-stream ordering.  Measured on MI355X (tools/sync_lab.hip, profiles/r02/sync_lab.txt): one exchange-shaped
  // dependency pair costs 15 us of stream time with hipEventRecord / hipStreamWaitEvent and 9 us with
  // hipStreamWriteValue64 / hipStreamWaitValue64 on a device flag; the latter is used where the device supports it.
  uint64_t* flags = nullptr;             // 2 * NEV counters, one cache line each
  uint64_t epoch = 0;
  bool use_values = false;
  // Whole-cycle graph.  At strong-scaling sizes (1.25 M rows per rank and below) one application is ~30 launches, three
  // RCCL groups and six cross-stream orderings for 100 - 200 us of GPU work: the host cannot enqueue them faster than the
  // GPU retires them.  The collective cycle -- both streams, pack kernels and ncclSend / ncclRecv / ncclAllGather
  // included -- is therefore captured ONCE per (b, x, b_status) into a hipGraph (cross-stream orderings become graph edges,
  // i.e. cost nothing at replay) and replayed with one launch.  AMGX_DIST_GRAPH=0 keeps direct launches; a capture that
  // fails (a runtime / RCCL build that cannot capture an operation) falls back to direct launches for good.
  bool graph_ok = true, capturing = false;
  struct GKey { std::vector<const void*> p; int status; bool operator<(const GKey& o) const { return status != o.status ? status < o.status : p < o.p; } };
  using Graphs = GraphCache<GKey, int64_t>;
  Graphs graphs;                         // payload: the exchanges of one application, added to n_exchanges at every replay
  int64_t n_direct_runs = 0;             // applications launched directly; the first one always is (see dist_apply)
  int64_t n_graph_replays = 0;
  std::string graph_note;
  // workspace of amgx_dist_pcg / amgx_dist_gmres (DistKrylov), kept across solves so that its vector addresses -- the key of the
  // preconditioner's whole-cycle graph -- stay the same
  std::shared_ptr<void> krylov_ws;
  size_t krylov_members = 0;

  Comm() { for (int i = 0; i < NEV; ++i) { ev_ready[i] = nullptr; ev_done[i] = nullptr; } }
  ~Comm() {
    graphs.drop();
    for (int i = 0; i < NEV; ++i) { if (ev_ready[i]) (void)hipEventDestroy(ev_ready[i]); if (ev_done[i]) (void)hipEventDestroy(ev_done[i]); }
    if (flags) (void)hipFree(flags);
    if (nccl) (void)Rccl::get().CommDestroy(nccl);
    if (comm_stream) (void)hipStreamDestroy(comm_stream);
    if (own_compute) (void)hipStreamDestroy(own_compute);
  }
  void init_streams(const Knobs& K) {
    HIPCHK(hipSetDevice(device));
    HIPCHK(hipStreamCreateWithFlags(&own_compute, hipStreamNonBlocking));
    compute = own_compute;
    // the communication stream gets the higher priority: its small pack kernels and the RCCL kernels must not queue
    // behind the streaming kernels of the interior rows
    int lo = 0, hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
    HIPCHK(hipStreamCreateWithPriority(&comm_stream, hipStreamNonBlocking, hi));
    for (int i = 0; i < NEV; ++i) {
      HIPCHK(hipEventCreateWithFlags(&ev_ready[i], hipEventDisableTiming));
      HIPCHK(hipEventCreateWithFlags(&ev_done[i], hipEventDisableTiming));
    }
    int can = 0;
    if (hipDeviceGetAttribute(&can, hipDeviceAttributeCanUseStreamWaitValue, device) != hipSuccess) can = 0;
    use_values = can && !K.dist_events;
    graph_ok = K.dist_graph;
    if (use_values) {
      HIPCHK(hipMalloc((void**)&flags, 2 * NEV * 64));
      HIPCHK(hipMemset(flags, 0, 2 * NEV * 64));
    }
  }
  // everything enqueued on `from` so far happens before whatever is enqueued on `to` from now on
  // (while a graph is being captured the event form is used: it turns into a graph edge)
  void order(hipStream_t from, hipStream_t to, int slot, hipEvent_t ev) {
    if (use_values && !capturing) {
      uint64_t* f = flags + slot * 8;
      ++epoch;
      HIPCHK(hipStreamWriteValue64(from, f, epoch, 0));
      HIPCHK(hipStreamWaitValue64(to, f, epoch, hipStreamWaitValueGte, 0xffffffffffffffffull));
    } else {
      HIPCHK(hipEventRecord(ev, from));
      HIPCHK(hipStreamWaitEvent(to, ev, 0));
    }
  }
  // split form: the signal is enqueued now, the wait later (exchange_end)
  uint64_t signal(hipStream_t from, int slot, hipEvent_t ev) {
    if (use_values && !capturing) { ++epoch; HIPCHK(hipStreamWriteValue64(from, flags + slot * 8, epoch, 0)); return epoch; }
    HIPCHK(hipEventRecord(ev, from));
    return 0;
  }
  void wait(hipStream_t to, int slot, hipEvent_t ev, uint64_t value) {
    if (use_values && !capturing) HIPCHK(hipStreamWaitValue64(to, flags + slot * 8, value, hipStreamWaitValueGte, 0xffffffffffffffffull));
    else HIPCHK(hipStreamWaitEvent(to, ev, 0));
  }
  uint64_t done_value[NEV] = {0};

  // ---- halo exchange.  items[i] = (table, vector) of local member i.  Returns a ticket for exchange_end. -------------
  struct Item { HaloTable* t; double* vec; };

  // The wire.  Peer k of a rank has two segments: its share of the pack buffer (`sendbuf`, the rows this rank owns and the
  // peer keeps as ghosts) and its share of the vector's ghost block (the rows the peer owns).  `to_ghost`: every pack segment
  // travels into the ghost segment its peer keeps for this rank (owner -> ghost); otherwise every ghost segment travels into
  // the peer's pack segment (ghost -> owner).
  static int64_t seg_len(const HaloTable& t, size_t k, bool pack) { const auto& p = pack ? t.send_ptr : t.recv_ptr; return (p[k + 1] - p[k]) * t.bs; }
  static double* seg(const Item& it, size_t k, bool pack) {
    return pack ? it.t->sendbuf.p + it.t->send_ptr[k] * it.t->bs : it.vec + (it.t->n + it.t->recv_ptr[k]) * it.t->bs;
  }
  // RCCL: one group of sends and receives with this rank's peers (per peer the send first, on every rank)
  void wire_rccl(const Item& it, bool to_ghost) {
    Rccl& R = Rccl::get();
    const HaloTable& t = *it.t;
    if (t.peers.empty()) return;
    NCCLCHK(R.GroupStart());
    for (size_t k = 0; k < t.peers.size(); ++k) {
      const int64_t n_out = seg_len(t, k, to_ghost), n_in = seg_len(t, k, !to_ghost);
      if (n_out) NCCLCHK(R.Send(seg(it, k, to_ghost), (size_t)n_out, ncclDouble, t.peers[k], nccl, comm_stream));
      if (n_in) NCCLCHK(R.Recv(seg(it, k, !to_ghost), (size_t)n_in, ncclDouble, t.peers[k], nccl, comm_stream));
    }
    NCCLCHK(R.GroupEnd());
  }
  // local ranks: every source segment is copied into the matching segment of the peer
  void wire_local(const std::vector<Item>& items, bool to_ghost) {
    for (size_t i = 0; i < items.size(); ++i) {
      const HaloTable& t = *items[i].t;
      for (size_t k = 0; k < t.peers.size(); ++k) {
        const int q = t.peers[k];
        const int64_t len = seg_len(t, k, to_ghost);
        if (!len) continue;
        if (q < 0 || q >= (int)items.size()) throw Err("local exchange: peer out of range");
        const int kq = items[q].t->peer_pos((int)i);
        if (kq < 0 || seg_len(*items[q].t, kq, !to_ghost) != len) throw Err("local exchange: send / receive sizes do not match");
        dev_copy(seg(items[q], kq, !to_ghost), seg(items[i], k, to_ghost), len, comm_stream);
      }
    }
  }
  void wire(const std::vector<Item>& items, bool to_ghost) {
    if (kind == AMGX_COMM_RCCL) wire_rccl(items[0], to_ghost); else wire_local(items, to_ghost);
  }

  // owner -> ghost, overwrite (reference CO2CU: BufferM, send, ApplyG; dcc_map.cpp:138-178, 280-302)
  int exchange_begin(const std::vector<Item>& items) {
    Range rg("DCCMap::StartCO2CU");
    const int tk = ev_next; ev_next = (ev_next + 1) % NEV;
    ++n_exchanges;
    order(compute, comm_stream, tk, ev_ready[tk]);                 // everything the vectors depend on is enqueued
    for (const Item& it : items) {
      const int64_t len = it.t->n_send() * it.t->bs;
      if (len) launch(halo_pack_kernel, Handle::grid_for(len), BLOCK, 0, comm_stream, len, it.t->bs, it.t->send_idx.p, it.vec, it.t->sendbuf.p);
    }
    wire(items, true);
    done_value[tk] = signal(comm_stream, NEV + tk, ev_done[tk]);
    return tk;
  }
  void exchange_end(int ticket) { Range rg("DCCMap::ApplyCO2CU"); wait(compute, NEV + ticket, ev_done[ticket], done_value[ticket]); }

  // ghost -> owner, add, ghost entries zeroed afterwards (reference DIS2CO: BufferG, send, ApplyM; dcc_map.cpp:76-136, 249-274)
  void accumulate(const std::vector<Item>& items) {
    Range rg("DCCMap::StartDIS2CO");
    const int tk = ev_next; ev_next = (ev_next + 1) % NEV;
    ++n_exchanges;
    order(compute, comm_stream, tk, ev_ready[tk]);
    wire(items, false);
    for (const Item& it : items) {
      const HaloTable& t = *it.t;
      const int64_t gl = t.n_ghost * t.bs;
      if (gl) launch(halo_zero_kernel, Handle::grid_for(gl), BLOCK, 0, comm_stream, gl, it.vec + t.n * t.bs);
      for (size_t k = 0; k < t.peers.size(); ++k)            // one launch per peer: two peers may both contribute to a row
        if (const int64_t len = seg_len(t, k, true)) launch(halo_unpack_add_kernel, Handle::grid_for(len), BLOCK, 0, comm_stream, len, t.bs, t.send_idx.p + t.send_ptr[k], seg(it, k, true), it.vec);
    }
    order(comm_stream, compute, NEV + tk, ev_done[tk]);
  }
};

// ---------------------------------------------------------------------------------------------------
// one rank's share of a rank-partitioned hierarchy + the replicated tail
struct Dist {
  Comm* comm = nullptr;
  int index = 0;                         // position in comm->members
  std::unique_ptr<Handle> top, tail;
  int k = 0;                             // levels 0..k-1 smoothed in rank-partitioned form, level k gathered
  int sm_type = AMGX_SM_JACOBI;
  DistPath path = DistPath::JACOBI_FOLDED;   // the driver of the collective cycle; all members of a communicator agree
  bool overlap = true;                   // interior rows run beside the exchanges (orthogonal to the path)
  int cycle = AMGX_CYCLE_V;
  std::vector<HaloTable> halo;           // [k]
  std::vector<std::array<int, 4>> stage; // [k] colour ranges of the hybrid Gauss-Seidel stages: [s0,s1) first local part,
                                         //     [s1,s2) boundary ("EX") rows, [s2,s3) second local part (gssmoother.cpp:721-782)
  std::vector<char> send_early;          // [k] block-hybrid levels: every sent row lies in a boundary block, so the exchange of x
                                         //     may start while the interior blocks are still being swept
  std::vector<DevBuf<double>> bext, xext, text, rl;
  DevBuf<double> bk, bpad, bglob, xglob, xk_ext, x0;
  DevBuf<int64_t> kmap, compact;
  std::vector<int64_t> counts, offs;
  int64_t mcount = 0;                    // longest level-k piece
  bool force_allgather = false;
  amgx_handle_t* view_top = nullptr;     // see amgx_dist_handles
  amgx_handle_t* view_tail = nullptr;

  int64_t n(int l) const { return top->lev[l].len(); }
  // interior rows as the split launches see them: a level WITHOUT boundary rows (world size 1, or a rank whose piece touches no
  // other) reports "everything", so that the last partial slice / chunk is not left to an extra boundary launch (5 launches of
  // 4 ... 8 us per cycle at 108^3, profiles/r04/trace_dist_nv108_before.txt)
  int64_t n_int_span(int l) const { return halo[l].n_int >= top->lev[l].n ? (int64_t)1 << 60 : halo[l].n_int; }
  int64_t next(int l) const { return top->lev[l].ext_len(); }
};

static void dist_check_interior(const amgx_matrix& A, int64_t n_int) {
  for (int64_t i = 0; i < n_int; ++i)
    for (int64_t e = A.rowptr[i]; e < A.rowptr[i + 1]; ++e)
      if (A.col[e] >= A.n_rows) throw Err("rank-partitioned level: a row below n_interior has a ghost column");
}

static Dist* dist_create(Comm* c, const amgx_dist_desc* d, const Knobs& K) {
  if (!c || !d) throw Err("amgx_dist_create: null argument");
  if (c->kind == AMGX_COMM_RCCL && !c->members.empty()) throw Err("amgx_dist_create: an RCCL communicator carries one rank per process");
  if (c->kind == AMGX_COMM_LOCAL && (int)c->members.size() >= c->nranks) throw Err("amgx_dist_create: all local ranks exist already");
  const int self = c->kind == AMGX_COMM_RCCL ? c->rank : (int)c->members.size();
  if (d->rank != self) throw Err("amgx_dist_create: descriptor rank does not match the communicator (local ranks are created in order)");
  HIPCHK(hipSetDevice(c->device));
  auto D = std::make_unique<Dist>();
  D->comm = c;
  D->index = (int)c->members.size();
  D->k = d->top.n_levels - 1;
  if (D->k < 1) throw Err("amgx_dist_create: need at least one rank-partitioned level and the gathered level");
  if (!d->halo || !d->counts || !d->kmap) throw Err("amgx_dist_create: halo tables / level-k tables missing");
  D->sm_type = d->top.levels[0].sm_type;
  // Chebyshev levels are an opt-in of the descriptor (amgx_dist_desc.cheby): without it the type is refused as it always was
  if (!d->cheby)
    for (const amgx_hierarchy_desc* hd : {&d->top, &d->tail})
      for (int l = 0; l < hd->n_levels; ++l)
        if (hd->levels && hd->levels[l].sm_type == AMGX_SM_CHEBY)
          throw Err("amgx_dist_create: the Chebyshev smoother (AMGX_SM_CHEBY) on a rank-partitioned hierarchy is an opt-in: set amgx_dist_desc.cheby = 1");
  const bool fold = d->fold != 0;
  if (D->sm_type == AMGX_SM_CHEBY) {
    // Chebyshev on the rank-partitioned levels: every rank runs the same recurrence with the same coefficients, so
    // degree and ratio are those of level 0 everywhere (lambda_max may differ per level; without one it is estimated collectively)
    if (fold) throw Err("amgx_dist_create: fold is the V(1,1) Jacobi form (not available with the Chebyshev smoother)");
    const amgx_level_desc& s0 = d->top.levels[0];
    for (int l = 0; l < D->k; ++l) {
      const amgx_level_desc& s = d->top.levels[l];
      if (s.sm_type != AMGX_SM_CHEBY) continue;             // (refused below: all levels use the same smoother)
      if (s.cheb_degree != s0.cheb_degree || s.cheb_ratio != s0.cheb_ratio)
        throw Err("amgx_dist_create: all rank-partitioned levels must use the same cheb_degree and cheb_ratio (level " + std::to_string(l) + " differs from level 0)");
      if (s.mat_prec == AMGX_PREC_F32)
        throw Err("amgx_dist_create: level " + std::to_string(l) + ": mat_prec = AMGX_PREC_F32 is not available on rank-partitioned levels");
    }
  }
  for (int l = 0; l < D->k; ++l)
    if (d->top.levels[l].jacobi_prec != AMGX_JACOBI_PREC_F64)
      throw Err("amgx_dist_create: level " + std::to_string(l) + ": jacobi_prec is not available on rank-partitioned levels");
  bool generic = false, gsb = false;
  D->cycle = d->top.cycle;
  if (D->cycle != AMGX_CYCLE_V && D->cycle != AMGX_CYCLE_W) throw Err("amgx_dist_create: rank-partitioned hierarchies run V and W cycles");
  if (d->tail.cycle != d->top.cycle) throw Err("amgx_dist_create: the replicated tail must run the same cycle as the rank-partitioned levels");
  if (D->cycle == AMGX_CYCLE_W) generic = true;
  D->overlap = !K.dist_no_overlap;
  amgx_hierarchy_desc td = d->top;
  td.device = c->device; td.use_graph = 0; td.clev = AMGX_CLEV_NONE; td.coarse_n = 0; td.coarse_inv = nullptr;
  td.cycle = AMGX_CYCLE_V;                 // (the top handle is driven stage by stage: its own cycle type plays no role)
  D->top.reset(create(&td, K, -1));           // (driven stage by stage: no collapsed coarse levels)
  amgx_hierarchy_desc ld = d->tail;
  ld.device = c->device;
  D->tail.reset(create(&ld, K, 0));           // the replicated tail may collapse completely: x_glob = B b_glob in one GEMV
  // both handles work on the communicator's compute stream
  for (Handle* h : {D->top.get(), D->tail.get()}) { HIPCHK(hipStreamSynchronize(h->stream)); h->stream = c->compute; }
  const int k = D->k;
  D->halo.resize(k);
  D->stage.resize(k);
  for (int l = 0; l < k; ++l) {
    const amgx_level_desc& s = d->top.levels[l];
    if (s.sm_type != D->sm_type) throw Err("amgx_dist_create: all rank-partitioned levels must use the same smoother");
    if (s.sm_steps > 1 || s.sm_symm) generic = true;      // ProxySmoother on a rank-partitioned level (base_smoother.hpp:169-229)
    if (s.sm_steps != d->top.levels[0].sm_steps || s.sm_symm != d->top.levels[0].sm_symm) throw Err("amgx_dist_create: all rank-partitioned levels must use the same sm_steps / sm_symm");
    D->halo[l].build(d->halo[l], s.A.n_rows, s.A.n_cols, s.A.br, c->nranks, self);
    dist_check_interior(s.A, D->halo[l].n_int);
    if (fold && s.Q.rowptr) {           // the way up splits the same way: interior rows of Q must not read coarse ghosts
      const int64_t nco = d->top.levels[l + 1].A.n_rows;
      for (int64_t i = 0; i < D->halo[l].n_int; ++i)
        for (int64_t e = s.Q.rowptr[i]; e < s.Q.rowptr[i + 1]; ++e)
          if (s.Q.col[e] >= nco) throw Err("rank-partitioned level: a row of Q below n_interior reads a coarse ghost");
    }
    const int nc = s.sm_type == AMGX_SM_GS ? s.n_colors : (s.sm_type == AMGX_SM_BGS ? s.bgs_n_colors : 0);
    D->stage[l] = {0, 0, nc, nc};
    if (d->gs_stage && s.sm_type == AMGX_SM_GS) {
      const int32_t* g = d->gs_stage + 4 * l;
      if (!(g[0] == 0 && g[0] <= g[1] && g[1] <= g[2] && g[2] <= g[3] && g[3] == nc)) throw Err("amgx_dist_create: gs_stage must be 0 <= s1 <= s2 <= n_colors");
      D->stage[l] = {g[0], g[1], g[2], g[3]};
      // rows of the first and third stage must not read ghosts (they run while the exchange is in flight)
      for (int64_t i = 0; i < s.A.n_rows; ++i) {
        const int ci = s.color[i];
        if (ci < 0 || (ci >= g[1] && ci < g[2])) continue;
        for (int64_t e = s.A.rowptr[i]; e < s.A.rowptr[i + 1]; ++e)
          if (s.A.col[e] >= s.A.n_rows) throw Err("amgx_dist_create: a row of a local Gauss-Seidel stage has a ghost column");
      }
      // send side of the same contract: the exchange of x starts after the colours [s0, s2) and runs beside [s2, s3), so a
      // SENT row must have been swept by then.  Structurally symmetric matrices give that for free (a sent row reads a
      // ghost, hence sits in the boundary stage); for anything else the level runs without the overlap.
      const amgx_halo_desc& hd = d->halo[l];
      const int64_t ns = hd.n_peers > 0 ? hd.send_ptr[hd.n_peers] : 0;
      for (int64_t i = 0; i < ns; ++i)
        if (s.color[hd.send_idx[i]] >= g[2]) { D->stage[l] = {g[0], g[1], nc, nc}; break; }
    }
    D->send_early.push_back(1);
    if (const LevelPaths& lp = D->top->lev[l].paths; lp.hybrid()) {
      // block-hybrid form: the boundary blocks [n_int / B, end) are swept first, then x travels beside the interior blocks
      const amgx_halo_desc& hd = d->halo[l];
      const int64_t ns = hd.n_peers > 0 ? hd.send_ptr[hd.n_peers] : 0;
      if (lp.bgsb() && s.gs_block_ids) throw Err("amgx_dist_create: rank-partitioned block levels sweep runs of consecutive rows (no gs_block_ids)");
      if (lp.sweep == SWEEP_BGSB_BC) throw Err("amgx_dist_create: rank-partitioned block levels sweep in the hybrid form (no gs_block_color)");
      const int64_t first_bnd = (D->halo[l].n_int / lp.unit_rows) * lp.unit_rows;
      for (int64_t i = 0; i < ns; ++i)
        if (hd.send_idx[i] < first_bnd) { D->send_early[l] = 0; break; }
    }
  }
  if (fold && generic) throw Err("amgx_dist_create: fold is the V(1,1) Jacobi form (no sm_steps / sm_symm / W-cycle)");
  if (fold) {
    if (D->sm_type != AMGX_SM_JACOBI) throw Err("amgx_dist_create: fold needs Jacobi levels");
    for (int l = 0; l < k; ++l) if (!D->top->folded(D->top->lev[l])) throw Err("amgx_dist_create: fold requested but level " + std::to_string(l) + " has no Q");
  }
  if (D->sm_type == AMGX_SM_GS) {
    int on = 0;
    for (int l = 0; l < k; ++l) on += D->top->lev[l].paths.hybrid() ? 1 : 0;
    if (on != 0 && on != k) throw Err("amgx_dist_create: either all or none of the rank-partitioned Gauss-Seidel levels use gs_block_rows");
    gsb = on == k;
  }
  D->path = generic ? DistPath::STEPWISE
          : D->sm_type == AMGX_SM_CHEBY ? DistPath::CHEBY
          : D->sm_type == AMGX_SM_JACOBI ? (fold ? DistPath::JACOBI_FOLDED : DistPath::JACOBI_LITERAL)
          : gsb ? DistPath::GS_BLOCK_HYBRID : DistPath::GS_STAGED;
  D->bext.resize(k); D->xext.resize(k); D->text.resize(k); D->rl.resize(k);
  auto zalloc = [&](DevBuf<double>& b, int64_t len) { b.alloc((size_t)std::max<int64_t>(1, len)); HIPCHK(hipMemset(b.p, 0, std::max<int64_t>(1, len) * sizeof(double))); };
  for (int l = 0; l < k; ++l) {
    zalloc(D->bext[l], D->next(l)); zalloc(D->xext[l], D->next(l)); zalloc(D->rl[l], D->n(l));
    if (D->path != DistPath::JACOBI_FOLDED && D->path != DistPath::GS_STAGED) zalloc(D->text[l], D->next(l));     // (the others work out of place)
  }
  // level k: gathered in rank order
  D->counts.assign(d->counts, d->counts + c->nranks);
  D->offs.assign(c->nranks + 1, 0);
  for (int r = 0; r < c->nranks; ++r) { if (D->counts[r] < 0) throw Err("amgx_dist_create: negative count"); D->offs[r + 1] = D->offs[r] + D->counts[r]; D->mcount = std::max(D->mcount, D->counts[r]); }
  // AMGX_DIST_FORCE_ALLGATHER (tests, one-GPU rehearsals): world size 1 goes through ncclAllGather too instead of the copy
  // shortcut; "pad" additionally pretends the pieces differ in size (every slot is 5 rows longer than the longest piece), so
  // that the padded all-gather and the compaction kernel run
  if (K.dist_force_allgather) {
    D->force_allgather = true;
    if (K.dist_force_allgather == 2) D->mcount += 5;
  }
  const int bsk = D->top->lev[k].bs;
  if (D->counts[self] * bsk != D->n(k)) throw Err("amgx_dist_create: counts[rank] does not match level k");
  if (D->offs.back() * bsk != D->tail->lev[0].len()) throw Err("amgx_dist_create: the replicated tail does not match the gathered level");
  if (d->kmap_len != D->next(k)) throw Err("amgx_dist_create: kmap must cover level k [owned | ghost]");
  for (int64_t i = 0; i < d->kmap_len; ++i) if (d->kmap[i] < 0 || d->kmap[i] >= D->offs.back() * bsk) throw Err("amgx_dist_create: kmap out of range");
  D->kmap.upload(d->kmap, (size_t)d->kmap_len);
  zalloc(D->bk, D->mcount * bsk); zalloc(D->bglob, D->offs.back() * bsk); zalloc(D->xglob, D->offs.back() * bsk);
  zalloc(D->xk_ext, D->next(k)); zalloc(D->x0, D->n(0));
  bool equal = true;
  for (int r = 0; r < c->nranks; ++r) equal = equal && D->counts[r] == D->mcount;
  if (!equal && c->kind == AMGX_COMM_RCCL) {
    // ncclAllGather moves pieces of one size: pad to the longest piece, then drop the padding with one gather
    zalloc(D->bpad, D->mcount * bsk * c->nranks);
    std::vector<int64_t> ci((size_t)(D->offs.back() * bsk));
    for (int r = 0; r < c->nranks; ++r)
      for (int64_t i = 0; i < D->counts[r] * bsk; ++i) ci[D->offs[r] * bsk + i] = (int64_t)r * D->mcount * bsk + i;
    D->compact.upload(ci);
  }
  HIPCHK(hipDeviceSynchronize());
  return D.release();
}

// ---------------------------------------------------------------------------------------------------
// the collective cycle.  All members of the communicator advance stage by stage (one member under RCCL): every stage is a
// loop over the local ranks in member order -- kernels of virtual ranks serialise on the one GPU in that order, and the RCCL
// group calls keep theirs on every rank.
struct DistCycle {
  Comm& c;
  std::vector<Dist*>& M;
  std::vector<double*> x;                // level-0 solution vectors (device)
  std::vector<const double*> b0;         // level-0 right-hand sides
  const int k = M[0]->k;
  using Span = Handle::Span;

  template <class F>
  void each(F&& f) { for (size_t i = 0; i < M.size(); ++i) f(*M[i], i); }
  std::vector<Comm::Item> items(int l, int which) {      // which: 0 bext, 1 xext, 2 text
    std::vector<Comm::Item> it;
    for (Dist* d : M) it.push_back({&d->halo[l], which == 0 ? d->bext[l].p : which == 1 ? d->xext[l].p : d->text[l].p});
    return it;
  }
  double* xl(Dist& d, size_t i, int l) { return l == 0 ? x[i] : d.xext[l].p; }
  const double* bl(Dist& d, size_t i, int l) { return l == 0 ? b0[i] : (const double*)d.bext[l].p; }
  double* bnext(Dist& d, int l) { return l + 1 < k ? d.bext[l + 1].p : d.bk.p; }
  const double* xcoarse(Dist& d, int l) { return l + 1 < k ? d.xext[l + 1].p : d.xk_ext.p; }     // owned part first in both

  // The overlapped stage: rows(d, i, span) on every rank around the end of the exchange with ticket `tk` (tk < 0: none in
  // flight, one launch covers everything).  With Dist::overlap the interior rows run while the exchange travels and the
  // boundary rows after it; without it everything runs after it.  What `rows` launches decides how a span is cut: formats that
  // cannot be split run completely in the boundary part, and a level without boundary rows reports everything as interior
  // (Dist::n_int_span), so that its boundary part is empty.
  template <class F>
  void overlapped(int l, int tk, F&& rows) {
    const bool split = tk >= 0 && M[0]->overlap;
    if (split) each([&](Dist& d, size_t i) { rows(d, i, Span{Handle::PART_INT, d.n_int_span(l)}); });
    if (tk >= 0) c.exchange_end(tk);
    each([&](Dist& d, size_t i) { rows(d, i, split ? Span{Handle::PART_BND, d.n_int_span(l)} : Span()); });
  }

  void gather_level_k() {
    each([&](Dist& d, size_t i) {
      const int bsk = d.top->lev[k].bs;
      if (c.kind == AMGX_COMM_RCCL) {
        Rccl& R = Rccl::get();
        if (c.nranks == 1 && !d.force_allgather) d.top->copy(d.bglob.p, d.bk.p, d.n(k));
        else if (d.compact.n == 0) NCCLCHK(R.AllGather(d.bk.p, d.bglob.p, (size_t)(d.mcount * bsk), ncclDouble, c.nccl, c.compute));
        else {
          NCCLCHK(R.AllGather(d.bk.p, d.bpad.p, (size_t)(d.mcount * bsk), ncclDouble, c.nccl, c.compute));
          const int64_t len = d.offs.back() * bsk;
          launch(index_gather_kernel, Handle::grid_for(len), BLOCK, 0, c.compute, len, d.compact.p, d.bpad.p, d.bglob.p);
        }
      } else {
        for (size_t q = 0; q < M.size(); ++q)
          if (d.counts[i]) dev_copy(M[q]->bglob.p + d.offs[i] * bsk, d.bk.p, d.counts[i] * bsk, c.compute);
      }
    });
  }
  // level k: gather the pieces, run the replicated tail, pick this rank's [owned | ghost] entries of its solution
  void tail() {
    gather_level_k();
    each([&](Dist& d, size_t) {
      // replicated tail: direct launches by default -- a graph launch between directly launched kernels costs ~10 us of
      // stream time (profiles/r02/trace_dist_world1.txt), the tail's handful of kernels do not pay that back
      d.tail->run_cycle(d.xglob.p, d.bglob.p, d.tail->knobs.dist_tail_graph && !c.capturing);
      const int64_t len = d.next(k);
      if (len) launch(index_gather_kernel, Handle::grid_for(len), BLOCK, 0, c.compute, len, d.kmap.p, d.xglob.p, d.xk_ext.p);
    });
  }

  // ---- Jacobi, post-smoothing folded into the prolongation: 2k - 1 exchanges.  The exchange of x_l started
  //      on the way up ends inside the stage of level l - 1 (the deferred ticket) ----------------------------------------
  void jacobi_folded() {
    for (int l = 0; l < k; ++l)
      overlapped(l, c.exchange_begin(items(l, 0)), [&](Dist& d, size_t i, Span sp) {
        d.top->pre_smooth_restrict(l, xl(d, i, l), d.bext[l].p, d.rl[l].p, bnext(d, l), true, sp);
      });
    tail();
    int tk = -1;
    for (int l = k - 1; l >= 0; --l) {
      overlapped(l, tk, [&](Dist& d, size_t i, Span sp) { d.top->post_smooth(l, xl(d, i, l), nullptr, d.rl[l].p, xcoarse(d, l), true, sp); });
      tk = l > 0 ? c.exchange_begin(items(l, 1)) : -1;
    }
  }

  // ---- Jacobi, literal stage order (base_smoother.cpp:61-74 around dof_map.cpp:636-709): 2k exchanges ----------------
  void jacobi_literal() {
    for (int l = 0; l < k; ++l)
      overlapped(l, c.exchange_begin(items(l, 0)), [&](Dist& d, size_t i, Span sp) {
        d.top->pre_smooth(d.top->lev[l], xl(d, i, l), d.bext[l].p, d.rl[l].p, false, sp);
        if (sp.part != Handle::PART_INT) d.top->transfer_f2c(l, d.rl[l].p, bnext(d, l));      // (once the rank's residual is complete)
      });
    tail();
    for (int l = k - 1; l >= 0; --l) {
      each([&](Dist& d, size_t i) { d.top->mult_add(d.top->lev[l].P, 1.0, xcoarse(d, l), xl(d, i, l), d.text[l].p); });
      overlapped(l, c.exchange_begin(items(l, 2)), [&](Dist& d, size_t i, Span sp) {
        d.top->jacobi_fused(d.top->lev[l], d.text[l].p, d.bext[l].p, xl(d, i, l), sp);
      });
    }
  }

  // ---- hybrid Gauss-Seidel: local sweeps with the off-rank values frozen at their sweep-start values (HybridGSSmoother,
  //      gssmoother.cpp:709-861).  Both drivers below run the same sequence -- sweep the part whose rows are sent, start the
  //      exchange of x, sweep the rest behind it, end it, residual + restriction; on the way up the mirror image around the
  //      exchange of x + P x_c -- and are kept as two: the staged form sweeps colour ranges in place (it zeroes the whole
  //      vector, prolongs in place, exchanges xext and finishes with the part it began with), the block form sweeps block ranges
  //      out of place (it zeroes the ghosts only, prolongs into text, exchanges text, has its own residual forms and carries
  //      the probe).  A description of the ranges and the sweep that covers both is longer than the two loops.
  //
  //      Block-hybrid form (scalar and square-block levels alike: Handle::sweep with a block range): the blocks of a sweep are
  //      independent of each other (couplings that leave a block -- ghost columns included -- use the sweep-start vector), so the boundary blocks are
  //      swept first, the exchange of x starts, and the interior blocks run behind it; on the way up the interior blocks
  //      run while x + P x_c travels.  Two launches per sweep instead of one per colour and stage.
  void hybrid_gsb() {
    // (a level with a sent row inside an interior block sweeps all its blocks before the exchange: see Dist::send_early)
    auto nbi = [&](Dist& d, int l) { return d.send_early[l] ? (int)(d.halo[l].n_int / d.top->lev[l].paths.unit_rows) : 0; };
    // the blocks [q0, q1) of the level (q1 < 0: up to the last one), from x = 0 and backward on x + P x_c
    auto sweep_zero = [&](Dist& d, size_t i, int l, int q0, int q1) {
      d.top->sweep_from_zero(d.top->lev[l], d.xext[l].p, bl(d, i, l), d.rl[l].p, {q0, q1});
    };
    auto sweep_back = [&](Dist& d, size_t i, int l, int q0, int q1) {
      d.top->sweep(d.top->lev[l], 1, d.text[l].p, xl(d, i, l), bl(d, i, l), {q0, q1});
    };
    for (int l = 0; l < k; ++l) {
      each([&](Dist& d, size_t i) {
        d.top->zero(d.xext[l].p + d.n(l), d.next(l) - d.n(l));
        sweep_zero(d, i, l, nbi(d, l), -1);
      });
      const int tk = c.exchange_begin(items(l, 1));
      each([&](Dist& d, size_t i) { sweep_zero(d, i, l, 0, nbi(d, l)); });
      c.exchange_end(tk);
      each([&](Dist& d, size_t i) { d.top->residual_restrict_after_zero(l, d.xext[l].p, bl(d, i, l), d.rl[l].p, bnext(d, l)); });
    }
    tail();
    for (int l = k - 1; l >= 0; --l) {
      each([&](Dist& d, size_t) { d.top->mult_add(d.top->lev[l].P, 1.0, xcoarse(d, l), d.xext[l].p, d.text[l].p); });
      const int tk = c.exchange_begin(items(l, 2));
      each([&](Dist& d, size_t i) {
        // (amgx_dist_time_kernel, op 9: HIP events around the interior blocks' launch of the first local rank)
        const bool probe = i == 0 && d.top->probe_level == l && d.top->probe_kind == 9 && d.top->probe_e0;
        d.top->probed(probe, [&] { sweep_back(d, i, l, 0, nbi(d, l)); });
      });
      c.exchange_end(tk);
      each([&](Dist& d, size_t i) { sweep_back(d, i, l, nbi(d, l), -1); });
    }
  }

  //      Staged multicolour form: stages LOC_1 / EX / LOC_2 = colour ranges (gssmoother.cpp:721-782)
  void sweep(Dist& d, size_t i, int l, int dir, int c0, int c1) {
    if (c1 > c0) d.top->sweep(d.top->lev[l], dir, d.xext[l].p, nullptr, bl(d, i, l), {c0, c1});
  }
  void hybrid_gs() {
    for (int l = 0; l < k; ++l) {
      // pre: x = 0; forward sweep (all off-rank values are 0, no exchange needed before it); the owner -> ghost exchange
      // of x starts as soon as the boundary stage is done and hides behind the second local stage
      each([&](Dist& d, size_t i) {
        d.top->zero(d.xext[l].p, d.next(l));
        sweep(d, i, l, 0, d.stage[l][0], d.stage[l][2]);
      });
      const int tk = c.exchange_begin(items(l, 1));
      each([&](Dist& d, size_t i) { sweep(d, i, l, 0, d.stage[l][2], d.stage[l][3]); });
      c.exchange_end(tk);
      each([&](Dist& d, size_t i) {
        d.top->residual(d.top->lev[l].A, d.xext[l].p, bl(d, i, l), d.rl[l].p);
        d.top->transfer_f2c(l, d.rl[l].p, bnext(d, l));
      });
    }
    tail();
    for (int l = k - 1; l >= 0; --l) {
      each([&](Dist& d, size_t) { d.top->mult_add(d.top->lev[l].P, 1.0, xcoarse(d, l), d.xext[l].p, d.xext[l].p); });
      // post: backward sweep = the stages in reverse order; the exchange hides behind the (reversed) second local stage
      const int tk = c.exchange_begin(items(l, 1));
      each([&](Dist& d, size_t i) { sweep(d, i, l, 1, d.stage[l][2], d.stage[l][3]); });
      c.exchange_end(tk);
      each([&](Dist& d, size_t i) {
        sweep(d, i, l, 1, d.stage[l][0], d.stage[l][2]);
        if (l == 0) d.top->copy(x[i], d.xext[0].p, d.n(0));
      });
    }
  }

  // ---- Chebyshev.  One smooth is the schedule of cheb_schedule.hpp on the global operator: a product step
  //      reads the iterate on [owned | ghost] and writes owned rows, d lives on owned rows, and the owner -> ghost exchange of the
  //      iterate precedes every product step whose input ghosts are not known.  The order of the rows plays no role, so the
  //      result is the serial cycle's up to rounding.  The schedule is walked ONCE for all local ranks: its vectors are tokens,
  //      resolved per rank to the two [owned | ghost] buffers X / T the iterate ping-pongs between and to the level's d.
  //      first_all(out, c0): step 1 from zero on every rank, out(i) = rank i's buffer for x_1.  split: the interior rows of a
  //      product step run beside the exchange of its iterate.  Returns whether the result lies in T.
  template <class FirstAll>
  bool cheb_smooth(int l, ChebEntry entry, bool src_in_t, const std::vector<double*>& X, const std::vector<double*>& T, bool split,
                   bool ghosts_after_first, FirstAll&& first_all) {
    double tx = 0.0, tt = 0.0, td = 0.0;
    auto at = [&](const double* p, size_t i) { return p == &tx ? X[i] : T[i]; };
    const DevLevel& L0 = M[0]->top->lev[l];
    int tk = -1;
    auto first = [&](const double*, const double*, double* xout, double*, double c0) { first_all([&](size_t i) { return at(xout, i); }, c0); };
    auto exchange = [&](const double* v) {
      std::vector<Comm::Item> it;
      each([&](Dist& d, size_t i) { it.push_back({&d.halo[l], at(v, i)}); });
      tk = c.exchange_begin(it);
      if (!split) { c.exchange_end(tk); tk = -1; }
    };
    auto step = [&](const double* xin, double* xout, double c1, double c2, const double* d_old, double* d_new) {
      overlapped(l, tk, [&](Dist& d, size_t i, Span sp) {
        DevLevel& L = d.top->lev[l];
        d.top->cheb_step(L, at(xin, i), bl(d, i, l), at(xout, i), c1, c2, d_old ? L.d.p : nullptr, d_new ? L.d.p : nullptr, sp);
      });
      tk = -1;
    };
    const double* end = cheb_schedule(L0.cheb_degree, L0.cheb_c0, L0.cheb_c1, L0.cheb_c2, entry, nullptr, src_in_t ? &tt : &tx, &tx, &tt, &td,
                                      first, step, exchange, ghosts_after_first);
    return end == &tt;
  }

  //      The overlapped V(1,1) driver.  Per level and application 2 * degree exchanges:
  //        down  b (step 1 from zero is formed on the ghost rows too, from the exchanged b and the ghost entries of Dinv, so x_1
  //              travels nowhere); x_2 .. x_{degree-1} ahead of their product steps; x_degree ahead of the residual  = degree
  //        up    x + P x_c and x_1 .. x_{degree-1}, each ahead of its product step                                    = degree
  //      degree 1 is the literal Jacobi count.  The owned rows of step 1 run beside the exchange of b, the interior rows of every
  //      later pass beside the exchange of its iterate; with degree 1 the interior part of residual + restriction runs beside the
  //      exchange of b as well, and the ghost rows of x_1 are formed when it ends.  The iterate lives in xext / text; level 0
  //      copies out to the caller's x.
  void cheby() {
    std::vector<std::vector<double*>> X(k), T(k);
    for (int l = 0; l < k; ++l)
      for (Dist* d : M) { X[l].push_back(d->xext[l].p); T[l].push_back(d->text[l].p); }
    for (int l = 0; l < k; ++l) {
      const DevLevel& L0 = M[0]->top->lev[l];
      const int deg = L0.cheb_degree;
      const std::vector<double*>& X1 = *cheb_place(deg - 1, &X[l], &T[l]);            // where x_1 goes, so that x_degree lands in X
      int tk = c.exchange_begin(items(l, 0));
      auto ghost_rows = [&](Dist& d, size_t i) {
        const DevLevel& L = d.top->lev[l];
        d.top->cheb_first(L, bl(d, i, l), nullptr, X1[i], nullptr, L0.cheb_c0, L.n, L.ncols - L.n);
      };
      const bool in_t = cheb_smooth(l, ChebEntry::ZERO, false, X[l], T[l], true, true, [&](auto&& out, double c0) {
        each([&](Dist& d, size_t i) { d.top->cheb_first(d.top->lev[l], bl(d, i, l), nullptr, out(i), nullptr, c0); });
        if (deg > 1) { c.exchange_end(tk); tk = -1; each(ghost_rows); }      // (a product step follows: it reads the ghosts of x_1)
      });
      if (in_t) throw Err("rank-partitioned Chebyshev cycle: the iterate did not end in place");
      if (deg > 1) tk = c.exchange_begin(items(l, 1));
      overlapped(l, tk, [&](Dist& d, size_t i, Span sp) {
        Handle& h = *d.top;
        DevLevel& L = h.lev[l];
        if (deg == 1 && sp.part != Handle::PART_INT) ghost_rows(d, i);
        if (L.paths.down == DOWN_CHEB) h.down_launch(l, L.plan_rf, h.down_ops_cheb(d.xext[l].p, bl(d, i, l)), bnext(d, l), sp);
        else {
          h.residual_sm(L, d.xext[l].p, bl(d, i, l), d.rl[l].p, sp);
          if (sp.part != Handle::PART_INT) h.transfer_f2c(l, d.rl[l].p, bnext(d, l));
        }
      });
    }
    tail();
    for (int l = k - 1; l >= 0; --l) {
      const int deg = M[0]->top->lev[l].cheb_degree;
      const bool in_t = cheb_place(cheb_passes(deg, ChebEntry::ITERATE), &X[l], &T[l]) == &T[l];
      each([&](Dist& d, size_t i) { d.top->mult_add(d.top->lev[l].P, 1.0, xcoarse(d, l), d.xext[l].p, (in_t ? T[l] : X[l])[i]); });
      if (cheb_smooth(l, ChebEntry::ITERATE, in_t, X[l], T[l], true, false, [](auto&&, double) {})) throw Err("rank-partitioned Chebyshev cycle: the iterate did not end in place");
      if (l == 0) each([&](Dist& d, size_t i) { d.top->copy(x[i], d.xext[0].p, d.n(0)); });
    }
  }

  // ---- step-by-step driver: sm_steps / sm_symm (ProxySmoother, base_smoother.hpp:169-229: k x Smooth, or k x (Smooth + SmoothBack)
  //      for the pre- AND the post-smoothing) and the W-cycle (AMGMatrix::SmoothW, amg_matrix.cpp:37-107) on rank-partitioned
  //      levels.  Every smoothing step is one step of the parallel smoother (hybrid_base_smoother.cpp:246-289): owner -> ghost
  //      exchange of x, then the local step with the ghost values frozen (Jacobi: x + w Dinv (b - (M + G) x); Gauss-Seidel: the
  //      staged / block-hybrid sweep).  No interior / boundary overlap here: one exchange, one launch per step.
  struct GenState { std::vector<double*> cur, oth; };        // per level: the [owned | ghost] buffer that holds x, and the spare one
  std::vector<GenState> gx;
  void gen_exchange(int l) {
    std::vector<Comm::Item> it;
    each([&](Dist& d, size_t i) { it.push_back({&d.halo[l], gx[l].cur[i]}); });
    c.exchange_end(c.exchange_begin(it));
  }
  // Chebyshev: one step is one smooth of the level's degree -- the schedule with an exchange ahead of every product step (step 1
  // from zero covers owned rows only here, so x_1 travels) and no overlap; the result is wherever the last pass left it
  void gen_cheb(int l, bool x_zero) {
    const bool in_t = cheb_smooth(l, x_zero ? ChebEntry::ZERO : ChebEntry::ITERATE, false, gx[l].cur, gx[l].oth, false, false, [&](auto&& out, double c0) {
      each([&](Dist& d, size_t i) { d.top->cheb_first(d.top->lev[l], bl(d, i, l), nullptr, out(i), nullptr, c0); });
    });
    if (in_t) std::swap(gx[l].cur, gx[l].oth);
  }
  void gen_step(int l, int dir, bool x_zero) {
    if (M[0]->sm_type == AMGX_SM_CHEBY) { gen_cheb(l, x_zero); return; }
    if (!x_zero) gen_exchange(l);                             // (from x = 0 the ghost values are zeros already)
    each([&](Dist& d, size_t i) {
      Handle& h = *d.top;
      DevLevel& L = h.lev[l];
      double*& cur = gx[l].cur[i];
      double*& oth = gx[l].oth[i];
      const double* b = bl(d, i, l);
      if (d.sm_type == AMGX_SM_JACOBI) { h.jacobi_fused(L, cur, b, oth); std::swap(cur, oth); }
      else if (h.sweep(L, dir, cur, oth, b) == oth) std::swap(cur, oth);       // (the out-of-place forms leave x in the spare buffer)
    });
  }
  // sm_steps steps in direction dir, or sm_steps x (forward, backward) with sm_symm
  void gen_smooth(int l, int dir, bool x_zero) {
    const DevLevel& L0 = M[0]->top->lev[l];
    const int steps = std::max(1, L0.sm_steps);
    for (int j = 0; j < steps; ++j) {
      if (L0.sm_symm) { gen_step(l, 0, x_zero && j == 0); gen_step(l, 1, false); }
      else gen_step(l, dir, x_zero && j == 0);
    }
  }
  // one level and everything below it, `visits` times: 1 = V, 2 = W (Handle::w_rec on rank-partitioned levels)
  void gen_cycle(int l, int visits) {
    if (l == k) { tail(); return; }
    each([&](Dist& d, size_t i) { d.top->zero(gx[l].cur[i], d.next(l)); });
    for (int v = 0; v < visits; ++v) {
      gen_smooth(l, 0, v == 0);
      gen_exchange(l);                                         // r = b - (M + G) x, b_{l+1} = P^T r  (P is rank-local: no exchange)
      each([&](Dist& d, size_t i) {
        d.top->residual(d.top->lev[l].A, gx[l].cur[i], bl(d, i, l), d.rl[l].p);
        d.top->transfer_f2c(l, d.rl[l].p, bnext(d, l));
      });
      gen_cycle(l + 1, visits);
      each([&](Dist& d, size_t i) {                            // x_l += P x_{l+1}  (x_{l+1} is wherever the steps below left it)
        const double* xc = l + 1 < k ? (const double*)gx[l + 1].cur[i] : (const double*)d.xk_ext.p;
        d.top->mult_add(d.top->lev[l].P, 1.0, xc, gx[l].cur[i], gx[l].cur[i]);
      });
      gen_smooth(l, 1, false);
    }
  }
  void stepwise() {
    gx.assign(k, GenState());
    for (int l = 0; l < k; ++l)
      for (Dist* d : M) { gx[l].cur.push_back(d->xext[l].p); gx[l].oth.push_back(d->text[l].p); }
    gen_cycle(0, M[0]->cycle == AMGX_CYCLE_W ? 2 : 1);
    each([&](Dist& d, size_t i) { d.top->copy(x[i], gx[0].cur[i], d.n(0)); });
  }

  void run() {
    switch (M[0]->path) {
      case DistPath::JACOBI_FOLDED: jacobi_folded(); break;
      case DistPath::JACOBI_LITERAL: jacobi_literal(); break;
      case DistPath::GS_BLOCK_HYBRID: hybrid_gsb(); break;
      case DistPath::GS_STAGED: hybrid_gs(); break;
      case DistPath::STEPWISE: stepwise(); break;
      case DistPath::CHEBY: cheby(); break;
    }
  }
};

// lambda_max(Dinv A) of the rank-partitioned Chebyshev levels that got none: the estimator of cheb_estimate (amgx.hip) on the
// partitioned operator -- 30 steps, 1.1 x the last Rayleigh quotient.  The start vector is fill_kernel(seed 1) at every rank's
// LOCAL scalar index; an owner -> ghost exchange of the operand precedes each product; the two dot products are deterministic
// local reductions, summed over the local ranks in member order by one kernel and over the processes by one all-reduce of two
// scalars.  The break-or-continue decision is taken on the reduced values, so every rank -- one without rows included -- takes
// the same branch and ends with bitwise the same interval.  Collective; runs once per communicator, before the first
// application (the coefficients are kernel arguments: a captured cycle has them baked in).
static void dist_cheb_estimate(Comm& c) {
  if (c.cheb_estimate_done) return;
  std::vector<Dist*>& M = c.members;
  if (M.empty() || (c.kind == AMGX_COMM_LOCAL && (int)M.size() != c.nranks)) throw Err("amgx_dist_cheb_estimate: not all ranks have a hierarchy");
  const size_t R = M.size();
  DevBuf<double> partial, sc;
  for (int l = 0; l < M[0]->k; ++l) {
    if (M[0]->top->lev[l].sm_type != AMGX_SM_CHEBY) continue;
    const bool given = M[0]->top->lev[l].cheb_lmax > 0.0;
    for (Dist* d : M) if ((d->top->lev[l].cheb_lmax > 0.0) != given) throw Err("amgx_dist_cheb_estimate: level " + std::to_string(l) + ": cheb_lambda_max is set on some ranks only");
    if (given) continue;
    if (!partial.p) { partial.alloc((size_t)2 * KR_BLOCKS * R); sc.alloc(2); }
    HIPCHK(hipMemsetAsync(partial.p, 0, (size_t)2 * KR_BLOCKS * R * sizeof(double), c.compute));   // (slots a short rank never writes)
    // work vectors of rank i: v = x, t = res, w = tmp of its level (v and w carry ghost entries)
    auto halo = [&](bool of_w) {
      std::vector<Comm::Item> it;
      for (Dist* d : M) it.push_back({&d->halo[l], of_w ? d->top->lev[l].tmp.p : d->top->lev[l].x.p});
      c.exchange_end(c.exchange_begin(it));
    };
    for (Dist* d : M) {
      DevLevel& L = d->top->lev[l];
      if (L.len()) launch(fill_kernel, Handle::grid_for(L.len()), BLOCK, 0, c.compute, L.len(), (uint64_t)1, L.tmp.p);
    }
    halo(true);
    for (Dist* d : M) {
      DevLevel& L = d->top->lev[l];
      d->top->mult(L.A, L.tmp.p, L.res.p);
      d->top->cheb_first(L, L.res.p, nullptr, L.x.p, nullptr, 1.0);
    }
    double lam = 0.0;
    for (int it = 0; it < 30; ++it) {
      halo(false);
      for (size_t i = 0; i < R; ++i) {
        Handle& h = *M[i]->top;
        DevLevel& L = h.lev[l];
        const int64_t n = L.len();
        h.mult(L.A, L.x.p, L.res.p);
        h.cheb_first(L, L.res.p, nullptr, L.tmp.p, nullptr, 1.0);
        if (!n) continue;
        const int nb = (int)std::max<int64_t>(1, std::min<int64_t>(KR_BLOCKS, (n + BLOCK - 1) / BLOCK));
        launch(kr_dot_partial_kernel, nb, BLOCK, 0, c.compute, n, (const double*)L.res.p, (const double*)L.tmp.p, partial.p + i * KR_BLOCKS);
        launch(kr_dot_partial_kernel, nb, BLOCK, 0, c.compute, n, (const double*)L.res.p, (const double*)L.x.p, partial.p + (R + i) * KR_BLOCKS);
      }
      launch(kr_dot_final_kernel, 1, BLOCK, 0, c.compute, (int)(KR_BLOCKS * R), (const double*)partial.p, sc.p);
      launch(kr_dot_final_kernel, 1, BLOCK, 0, c.compute, (int)(KR_BLOCKS * R), (const double*)(partial.p + R * KR_BLOCKS), sc.p + 1);
      if (c.kind == AMGX_COMM_RCCL && (c.nranks > 1 || M[0]->force_allgather))
        NCCLCHK(Rccl::get().AllReduce(sc.p, sc.p, 2, ncclDouble, ncclSum, c.nccl, c.compute));
      double two[2] = {0.0, 0.0};
      HIPCHK(hipMemcpyAsync(two, sc.p, 2 * sizeof(double), hipMemcpyDeviceToHost, c.compute));
      HIPCHK(hipStreamSynchronize(c.compute));
      if (!(two[1] > 0.0) || !(two[0] > 0.0) || !std::isfinite(two[0] / two[1])) break;      // A v = 0 (no free row): keep the last value
      lam = two[0] / two[1];
      for (Dist* d : M) {
        DevLevel& L = d->top->lev[l];
        if (L.len()) launch(kr_scale_kernel, Handle::grid_for(L.len()), BLOCK, 0, c.compute, L.len(), 1.0 / lam, (const double*)L.tmp.p, L.x.p, 0);
      }
    }
    if (!(lam > 0.0)) lam = 1.0;
    for (Dist* d : M) {
      DevLevel& L = d->top->lev[l];
      L.cheb_set_interval(1.1 * lam);
      L.cheb_estimated = 1;
      const size_t len = (size_t)std::max<int64_t>(1, L.ext_len());
      for (double* q : {L.x.p, L.res.p, L.tmp.p}) HIPCHK(hipMemsetAsync(q, 0, len * sizeof(double), c.compute));
    }
    HIPCHK(hipStreamSynchronize(c.compute));
    HIPCHK(hipStreamSynchronize(c.comm_stream));
  }
  c.cheb_estimate_done = true;
}

// b_status 0 (DISTRIBUTED): b carries [owned | ghost] entries and the ghost entries are contributions to their owners
// (b.Distribute() state of the reference, amg_matrix.cpp:164); 1 (CUMULATED): the owned entries are complete.
static void dist_apply(Comm& c, const double* const* b, double* const* x, int b_status, int flags) {
  Range rg("AMGMatrix::Mult");
  std::vector<Dist*>& M = c.members;
  if (M.empty()) throw Err("amgx_dist_apply: the communicator has no rank-partitioned hierarchy");
  if (c.kind == AMGX_COMM_LOCAL && (int)M.size() != c.nranks) throw Err("amgx_dist_apply: not all local ranks have been created");
  if (!b || !x) throw Err("amgx_dist_apply: null vector list");
  dist_cheb_estimate(c);                  // (does nothing after the first call)
  const bool host = !(flags & AMGX_DEVICE_PTR);
  for (size_t i = 0; i < M.size(); ++i)
    if ((!b[i] || !x[i]) && M[i]->n(0) > 0) throw Err("amgx_dist_apply: null vector");
  auto body = [&]() {
    DistCycle cy{c, M};
    for (size_t i = 0; i < M.size(); ++i) {
      Dist* d = M[i];
      const int64_t nb = b_status == 0 ? d->next(0) : d->n(0);
      if (nb == 0) {}
      else if (host) HIPCHK(hipMemcpyAsync(d->bext[0].p, b[i], nb * sizeof(double), hipMemcpyHostToDevice, c.compute));
      else if (b[i] != d->bext[0].p) dev_copy(d->bext[0].p, b[i], nb, c.compute);
      cy.b0.push_back(d->bext[0].p);
      cy.x.push_back(host ? d->x0.p : x[i]);
    }
    if (b_status == 0) c.accumulate(cy.items(0, 0));
    cy.run();
  };
  // ---- replay / capture of the whole collective cycle (see Comm::graphs) ----------------------------------------------
  if (c.graph_ok && !host && !(flags & AMGX_NO_GRAPH) && c.compute != nullptr) {
    Comm::GKey key;
    key.status = b_status;
    for (size_t i = 0; i < M.size(); ++i) { key.p.push_back(b[i]); key.p.push_back(x[i]); }
    auto* g = c.graphs.find(key);
    // The FIRST application of a communicator is always launched directly: RCCL sets up its point-to-point and all-gather
    // connections lazily inside the first calls, which must not happen inside a stream capture; the capture starts with the
    // second application, when every connection exists.
    if (!g && c.n_direct_runs > 0) {
      // relaxed capture: the communication stream joins the capture through the first cross-stream ordering and is joined
      // back by the last exchange_end / accumulate, as hipStreamEndCapture requires
      const int64_t ex0 = c.n_exchanges;
      Comm::Graphs::Failure why;
      c.capturing = true;
      g = c.graphs.capture(key, c.compute, hipStreamCaptureModeRelaxed, body, why);
      c.capturing = false;
      const int64_t nex = c.n_exchanges - ex0;              // counted while capturing; from now on added per replay
      c.n_exchanges = ex0;
      if (g) g->payload = nex;
      else {      // the capture did not work out: never try again on this communicator, run this application directly
        c.graph_ok = false;
        c.graph_note = "whole-cycle graph capture failed (" + why.text() + "): direct launches";
      }
    }
    if (g) {
      HIPCHK(hipGraphLaunch(g->exec, c.compute));
      c.n_exchanges += g->payload;
      ++c.n_graph_replays;
      return;
    }
  }
  ++c.n_direct_runs;
  body();
  if (host) {
    for (size_t i = 0; i < M.size(); ++i)
      if (M[i]->n(0)) HIPCHK(hipMemcpyAsync(x[i], M[i]->x0.p, M[i]->n(0) * sizeof(double), hipMemcpyDeviceToHost, c.compute));
    HIPCHK(hipStreamSynchronize(c.compute));
  }
}

// ---------------------------------------------------------------------------------------------------
// The Krylov solvers of krylov_core.hpp over the rank-partitioned level-0 operator (SURVEY.md 8f-3 for several ranks).  On the
// reference side these are NGSolve's CGSolver / GMRes on ParallelVectors (tests/h1/amg_utils.py:337-363): every rank runs the
// recurrences on its owned entries, the level-0 product needs the ghost values of its operand (one owner -> ghost exchange,
// hidden behind the interior rows), every inner product is a sum over the ranks (MPI all-reduce there; ncclAllReduce of the
// device scalars here, deterministic local reductions), the preconditioner is the collective cycle (dist_apply, replayed from
// its graph).
// out[j] = sum over the local ranks i and their KR_BLOCKS partials of product j (partial laid out [rank][64][KR_BLOCKS]); fixed order
__global__ __launch_bounds__(BLOCK) void kr_dist_multi_final_kernel(int n_local, const double* __restrict__ partial, double* __restrict__ out) {
  __shared__ double red[BLOCK];
  const int j = blockIdx.x;
  double acc = 0.0;
  for (int i = 0; i < n_local; ++i) {
    const double* p = partial + ((size_t)i * 64 + j) * KR_BLOCKS;
    for (int q = threadIdx.x; q < KR_BLOCKS; q += BLOCK) acc += p[q];
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int o = BLOCK >> 1; o > 0; o >>= 1) { if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o]; __syncthreads(); }
  if (threadIdx.x == 0) out[j] = red[0];
}

// The rank space of krylov_core.hpp: a vector is one pointer per local rank (owned entries).  The residual role is the cycle's
// level-0 right-hand-side buffer, so the preconditioner reads it in place; the operand role is the [owned | ghost] buffer the
// level-0 product reads, so CG's direction and the single-reduction form's u are multiplied in place.  Any other vector is
// copied there first (Handle::copy does nothing when source and destination are the same).  Kept with the communicator
// (Comm::krylov_ws).  A rank without rows launches nothing element-wise; its buffers have one entry.
struct DistKrylov {
  struct Vec { double* const* p; int64_t col; };             // rank i: p[i] + col * (its owned entries); col != 0 only in the basis
  struct CVec { const double* const* p; int64_t col; CVec(const double* const* pp) : p(pp), col(0) {} CVec(Vec v) : p(v.p), col(v.col) {} };
  using Bufs = std::vector<DevBuf<double>>;
  Comm& c;
  std::vector<Dist*>& M;
  const size_t R;
  Bufs sext, w;                                  // operand of A [owned | ghost], work vector (owned)
  Bufs sr_p, sr_s;                               // single-reduction form: p, s
  Bufs gV, gt;                                   // GMRES: basis (m + 1) x n_owned, work vector
  DevBuf<double> partial, sr_partial, gpartial;  // partial sums of dot / sr_reduce / multi_dot, each zeroed once: slots a short rank never writes stay 0
  DevBuf<double> sc, hdev;                       // device scalars; coefficients of basis_update
  int g_m = 0;
  enum { RES, OP, W0, W1, W2, BASIS, N_ROLES };
  std::vector<double*> rows[N_ROLES];            // what the Vec handles name: per role, one pointer per local rank (set by begin)
  explicit DistKrylov(Comm& cc) : c(cc), M(cc.members), R(cc.members.size()) {
    sext.resize(R); w.resize(R);
    for (size_t i = 0; i < R; ++i) {
      sext[i].alloc((size_t)std::max<int64_t>(1, M[i]->next(0)));
      w[i].alloc((size_t)std::max<int64_t>(1, n(i)));
      HIPCHK(hipMemsetAsync(sext[i].p, 0, std::max<int64_t>(1, M[i]->next(0)) * sizeof(double), c.compute));
    }
    partial.alloc((size_t)KR_BLOCKS * R);
    sc.alloc(64);
    HIPCHK(hipMemsetAsync(partial.p, 0, (size_t)KR_BLOCKS * R * sizeof(double), c.compute));
    HIPCHK(hipMemsetAsync(sc.p, 0, 64 * sizeof(double), c.compute));
  }
  int64_t n(size_t i) const { return M[i]->n(0); }
  Handle& top(size_t i) { return *M[i]->top; }
  static int nb(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>(KR_BLOCKS, (n + BLOCK - 1) / BLOCK)); }
  int grid(size_t i) const { return Handle::grid_for(n(i)); }
  double* at(Vec v, size_t i) const { return v.p[i] + v.col * n(i); }
  const double* at(CVec v, size_t i) const { return v.p[i] + v.col * n(i); }
  void name(int role, Bufs& b) { rows[role].resize(R); for (size_t i = 0; i < R; ++i) rows[role][i] = b[i].p; }
  void alloc_owned(Bufs& b, size_t vectors) { b.clear(); b.resize(R); for (size_t i = 0; i < R; ++i) b[i].alloc(vectors * (size_t)std::max<int64_t>(1, n(i))); }

  void begin(Form f, int restart) {
    rows[RES].resize(R);
    for (size_t i = 0; i < R; ++i) rows[RES][i] = M[i]->bext[0].p;        // residual = right-hand side of the cycle
    name(OP, sext); name(W0, w);
    if (f == Form::CG_SR) {
      if (sr_p.size() != R) {
        alloc_owned(sr_p, 1); alloc_owned(sr_s, 1);
        sr_partial.alloc((size_t)2 * KR_BLOCKS * R);
        HIPCHK(hipMemsetAsync(sr_partial.p, 0, (size_t)2 * KR_BLOCKS * R * sizeof(double), c.compute));
      }
      name(W1, sr_p); name(W2, sr_s);
    }
    if (f == Form::GMRES) {
      if (restart > 40) throw Err("amgx_dist_gmres: restart lengths above 40 are not supported (got " + std::to_string(restart) + ")");
      const int m = std::max(1, restart);
      if (g_m < m || gV.size() != R) {
        alloc_owned(gV, (size_t)(m + 1)); alloc_owned(gt, 1);
        gpartial.alloc((size_t)KR_BLOCKS * 64 * R);
        HIPCHK(hipMemsetAsync(gpartial.p, 0, (size_t)KR_BLOCKS * 64 * R * sizeof(double), c.compute));
        hdev.alloc(64);
        g_m = m;
      }
      name(W1, gt); name(BASIS, gV);
    }
  }
  Vec residual_vec() { return {rows[RES].data(), 0}; }
  Vec operand() { return {rows[OP].data(), 0}; }
  Vec work(int k) { return {rows[W0 + k].data(), 0}; }
  Vec basis(int j) { return {rows[BASIS].data(), j}; }

  // rows(i, span) for every rank behind the owner -> ghost exchange of the operand buffer: interior rows before it ends
  template <class F>
  void with_halo(F&& rows_of) {
    std::vector<Comm::Item> it;
    for (size_t i = 0; i < R; ++i) it.push_back({&M[i]->halo[0], sext[i].p});
    const int tk = c.exchange_begin(it);
    const bool ov = M[0]->overlap;
    if (ov) for (size_t i = 0; i < R; ++i) rows_of(i, Handle::Span{Handle::PART_INT, M[i]->n_int_span(0)});
    c.exchange_end(tk);
    for (size_t i = 0; i < R; ++i) rows_of(i, ov ? Handle::Span{Handle::PART_BND, M[i]->n_int_span(0)} : Handle::Span());
  }
  void residual(CVec x, CVec b, Vec r) {
    copy(operand(), x);
    with_halo([&](size_t i, Handle::Span sp) { top(i).residual(top(i).lev[0].A, sext[i].p, at(b, i), at(r, i), sp); });
  }
  void mult(CVec v, Vec y) {
    copy(operand(), v);
    with_halo([&](size_t i, Handle::Span sp) { top(i).mult(top(i).lev[0].A, sext[i].p, at(y, i), sp); });
  }
  void precond(CVec r, Vec z, bool use_pre) {
    copy(use_pre ? residual_vec() : z, r);
    if (!use_pre) return;
    std::vector<double*> xp(R);
    for (size_t i = 0; i < R; ++i) xp[i] = at(z, i);
    dist_apply(c, rows[RES].data(), xp.data(), 1, AMGX_DEVICE_PTR);
  }

  // (world 1: the all-reduce runs only when the collectives are forced)
  void all_reduce(int s, size_t count) {
    if (c.kind == AMGX_COMM_RCCL && (c.nranks > 1 || M[0]->force_allgather))
      NCCLCHK(Rccl::get().AllReduce(sc.p + s, sc.p + s, count, ncclDouble, ncclSum, c.nccl, c.compute));
  }
  void dot(CVec a, CVec b, int s) {
    for (size_t i = 0; i < R; ++i)
      if (n(i)) launch(kr_dot_partial_kernel, nb(n(i)), BLOCK, 0, c.compute, n(i), at(a, i), at(b, i), partial.p + i * KR_BLOCKS);
    launch(kr_dot_final_kernel, 1, BLOCK, 0, c.compute, (int)(KR_BLOCKS * R), partial.p, sc.p + s);
    all_reduce(s, 1);
  }
  void multi_dot(int m, CVec v) {
    if (m > 48) throw Err("multi_dot: too many vectors");
    for (size_t i = 0; i < R; ++i)
      if (n(i)) launch(kr_multi_dot_partial_kernel, nb(n(i)), BLOCK, 0, c.compute, n(i), m, gV[i].p, n(i), at(v, i), gpartial.p + i * 64 * KR_BLOCKS);
    launch(kr_dist_multi_final_kernel, m, BLOCK, 0, c.compute, (int)R, gpartial.p, sc.p);
    all_reduce(0, (size_t)m);
  }
  void sr_reduce(CVec r, CVec u, CVec v) {
    for (size_t i = 0; i < R; ++i)
      if (n(i)) launch(kr_dot2_partial_kernel, nb(n(i)), BLOCK, 0, c.compute, n(i), at(r, i), at(u, i), at(v, i), sr_partial.p + i * 2 * KR_BLOCKS);
    launch(kr_sr_reduce_kernel, 2, BLOCK, 0, c.compute, (int)R, sr_partial.p, sc.p);
    all_reduce(SR_GNEW, 2);
    launch(kr_sr_scalars_kernel, 1, 1, 0, c.compute, sc.p);
  }
  double read(int s) {
    double v = 0.0;
    read(s, 1, &v);
    return v;
  }
  void read(int s0, int m, double* out) {
    HIPCHK(hipMemcpyAsync(out, sc.p + s0, m * sizeof(double), hipMemcpyDeviceToHost, c.compute));
    HIPCHK(hipStreamSynchronize(c.compute));
  }
  void write(int s, double v) { HIPCHK(hipMemcpyAsync(sc.p + s, &v, sizeof(double), hipMemcpyHostToDevice, c.compute)); }

  void copy(Vec dst, CVec src) { for (size_t i = 0; i < R; ++i) top(i).copy(at(dst, i), at(src, i), n(i)); }
  void zero(Vec a, Vec b) { for (size_t i = 0; i < R; ++i) { top(i).zero(at(a, i), n(i)); top(i).zero(at(b, i), n(i)); } }
  void scale(double alpha, CVec x, Vec y) {
    for (size_t i = 0; i < R; ++i) if (n(i)) launch(kr_scale_kernel, grid(i), BLOCK, 0, c.compute, n(i), alpha, at(x, i), at(y, i), 0);
  }
  void cg_update(int num, int den, CVec s, CVec q, Vec x, Vec d) {
    for (size_t i = 0; i < R; ++i) if (n(i)) launch(kr_cg_update_kernel, grid(i), BLOCK, 0, c.compute, n(i), sc.p, num, den, at(s, i), at(q, i), at(x, i), at(d, i));
  }
  void xpby(int num, int den, CVec v, Vec s) {
    for (size_t i = 0; i < R; ++i) if (n(i)) launch(kr_xpby_kernel, grid(i), BLOCK, 0, c.compute, n(i), sc.p, num, den, at(v, i), at(s, i));
  }
  void sr_update(CVec u, CVec v, Vec p, Vec s, Vec x, Vec r) {
    for (size_t i = 0; i < R; ++i) if (n(i)) launch(kr_sr_update_kernel, grid(i), BLOCK, 0, c.compute, n(i), sc.p, at(u, i), at(v, i), at(p, i), at(s, i), at(x, i), at(r, i));
  }
  void basis_update(int m, const double* coef, double sign, Vec v) {
    HIPCHK(hipMemcpyAsync(hdev.p, coef, m * sizeof(double), hipMemcpyHostToDevice, c.compute));
    for (size_t i = 0; i < R; ++i) if (n(i)) launch(kr_multi_axpy_kernel, grid(i), BLOCK, 0, c.compute, n(i), m, gV[i].p, n(i), hdev.p, sign, at(v, i));
    HIPCHK(hipStreamSynchronize(c.compute));
  }
};

}  // namespace amgx

// ---------------------------------------------------------------------------------------------------
// C ABI (include/amgx.h, "rank-partitioned hierarchies")
// ---------------------------------------------------------------------------------------------------
struct amgx_comm_t { amgx::Comm* c; };
struct amgx_halo_t { amgx::Comm* c; amgx::HaloTable t; };

namespace {
template <class F>
int cguard(amgx_comm cc, F&& f) {
  try {
    if (!cc || !cc->c) throw amgx::Err("null communicator");
    HIPCHK(hipSetDevice(cc->c->device));
    f(*cc->c);
    return 0;
  } catch (const std::exception& e) {
    if (cc && cc->c) cc->c->err = e.what(); else g_create_err = e.what();
    return 1;
  }
}

// argument checks of the rank solvers.  fn: the entry point's name, so every Err text names its caller; bad_args: the entry
// point's own test of its scalar arguments (amgx_dist_gmres also rejects restart < 1), evaluated there because b and x are read
// here only after it; alias_note: what the entry point appends to the aliasing message (amgx_dist_pcg says why, amgx_dist_gmres "")
void check_dist_solve(const char* fn, amgx::Comm& c, bool bad_args, const double* const* b, double* const* x, int flags, const char* alias_note) {
  const std::string f(fn);
  if (bad_args) throw amgx::Err(f + ": bad arguments");
  if (!(flags & AMGX_DEVICE_PTR)) throw amgx::Err(f + ": device vectors only (AMGX_DEVICE_PTR)");
  if (c.members.empty() || (c.kind == AMGX_COMM_LOCAL && (int)c.members.size() != c.nranks)) throw amgx::Err(f + ": not all ranks have a hierarchy");
  for (size_t i = 0; i < c.members.size(); ++i) {
    amgx::Dist* d = c.members[i];
    if ((!b[i] || !x[i]) && d->n(0) > 0) throw amgx::Err(f + ": null vector");
    if (b[i] == d->bext[0].p || x[i] == d->bext[0].p) throw amgx::Err(f + ": b / x alias the cycle's right-hand-side buffer" + alias_note);
  }
  amgx::dist_cheb_estimate(c);
}
// the workspace lives with the communicator: the preconditioner's whole-cycle graph is keyed on the vector addresses, so a
// second solve replays the graph of the first instead of capturing a new one (and leaving a stale one behind)
amgx::DistKrylov& dist_krylov(amgx::Comm& c) {
  if (!c.krylov_ws || c.krylov_members != c.members.size()) {
    c.krylov_ws = std::shared_ptr<void>(new amgx::DistKrylov(c), [](void* p) { delete static_cast<amgx::DistKrylov*>(p); });
    c.krylov_members = c.members.size();
  }
  return *static_cast<amgx::DistKrylov*>(c.krylov_ws.get());
}
}  // namespace

extern "C" {

const char* amgx_comm_last_error(amgx_comm c) { return (c && c->c) ? c->c->err.c_str() : g_create_err.c_str(); }

int amgx_comm_unique_id(char* id128) {
  try {
    if (!id128) throw amgx::Err("amgx_comm_unique_id: null buffer");
    static_assert(sizeof(ncclUniqueId) == AMGX_UNIQUE_ID_BYTES, "ncclUniqueId size");
    ncclUniqueId id;
    NCCLCHK(amgx::Rccl::get().GetUniqueId(&id));
    std::memcpy(id128, &id, sizeof(id));
    return 0;
  } catch (const std::exception& e) { g_create_err = e.what(); return 1; }
}

int amgx_comm_create(int kind, int n_ranks, int rank, const char* id128, int device, amgx_comm* out) {
  try {
    if (!out) throw amgx::Err("amgx_comm_create: null output");
    if (kind != AMGX_COMM_RCCL && kind != AMGX_COMM_LOCAL) throw amgx::Err("amgx_comm_create: unknown kind");
    if (n_ranks < 1) throw amgx::Err("amgx_comm_create: n_ranks must be >= 1");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) throw amgx::Err("amgx_comm_create: no HIP device available (the apply path has no CPU fallback)");
    if (device < 0 || device >= ndev) throw amgx::Err("amgx_comm_create: device ordinal out of range");
    auto c = std::make_unique<amgx::Comm>();
    c->kind = kind; c->nranks = n_ranks; c->device = device;
    c->rank = kind == AMGX_COMM_RCCL ? rank : 0;
    c->init_streams(amgx::Knobs::from_env());
    if (kind == AMGX_COMM_RCCL) {
      if (rank < 0 || rank >= n_ranks || !id128) throw amgx::Err("amgx_comm_create: RCCL needs rank in [0, n_ranks) and the unique id of rank 0");
      ncclUniqueId id;
      std::memcpy(&id, id128, sizeof(id));
      NCCLCHK(amgx::Rccl::get().CommInitRank(&c->nccl, n_ranks, id, rank));     // collective over all ranks
    }
    *out = new amgx_comm_t{c.release()};
    return 0;
  } catch (const std::exception& e) { g_create_err = e.what(); return 1; }
}

int amgx_comm_destroy(amgx_comm c) {
  if (!c) return 0;
  if (c->c) {
    (void)hipSetDevice(c->c->device);
    (void)hipDeviceSynchronize();
    // wrappers stay allocated (a caller may still hold them) but point nowhere: amgx_dist_* / amgx_* calls through them fail cleanly
    for (amgx_dist_t* w : c->c->dist_wrappers) w->d = nullptr;
    for (amgx_handle_t* v : c->c->handle_views) v->h = nullptr;
    for (amgx::Dist* d : c->c->members) delete d;
    delete c->c;
  }
  delete c;
  return 0;
}

int amgx_comm_set_stream(amgx_comm cc, void* s) {
  return cguard(cc, [&](amgx::Comm& c) {
    hipStream_t ns = s ? (hipStream_t)s : c.own_compute;       // NULL: back to the communicator's own stream
    if (ns == c.compute) return;
    HIPCHK(hipStreamSynchronize(c.compute));
    HIPCHK(hipStreamSynchronize(c.comm_stream));
    c.compute = ns;
    c.graphs.drop();
    for (amgx::Dist* d : c.members) { d->top->drop_graphs(); d->tail->drop_graphs(); d->top->stream = ns; d->tail->stream = ns; }
  });
}

int amgx_comm_synchronize(amgx_comm cc) {
  return cguard(cc, [&](amgx::Comm& c) { HIPCHK(hipStreamSynchronize(c.comm_stream)); HIPCHK(hipStreamSynchronize(c.compute)); });
}

int amgx_comm_info(amgx_comm cc, int32_t* kind, int32_t* n_ranks, int32_t* rank, int64_t* n_exchanges) {
  return cguard(cc, [&](amgx::Comm& c) {
    if (kind) *kind = c.kind;
    if (n_ranks) *n_ranks = c.nranks;
    if (rank) *rank = c.rank;
    if (n_exchanges) *n_exchanges = c.n_exchanges;
  });
}

int amgx_comm_graph_info(amgx_comm cc, int32_t* enabled, int64_t* n_graphs, int64_t* n_replays) {
  return cguard(cc, [&](amgx::Comm& c) {
    if (enabled) *enabled = c.graph_ok ? 1 : 0;
    if (n_graphs) *n_graphs = (int64_t)c.graphs.size();
    if (n_replays) *n_replays = c.n_graph_replays;
  });
}
int amgx_comm_order_info(amgx_comm cc, int32_t* event_order) {
  return cguard(cc, [&](amgx::Comm& c) { if (event_order) *event_order = c.use_values ? 0 : 1; });
}
const char* amgx_comm_graph_note(amgx_comm c) { return (c && c->c) ? c->c->graph_note.c_str() : ""; }

int amgx_dist_create(amgx_comm cc, const amgx_dist_desc* desc, amgx_dist* out) {
  return cguard(cc, [&](amgx::Comm& c) {
    if (!out) throw amgx::Err("amgx_dist_create: null output");
    amgx::Dist* d = amgx::dist_create(&c, desc, amgx::Knobs::from_env());
    c.members.push_back(d);
    *out = new amgx_dist_t{d};
    c.dist_wrappers.push_back(*out);
  });
}

// the communicator owns the rank objects and their wrappers (freed / nulled by amgx_comm_destroy); nothing to do here
int amgx_dist_destroy(amgx_dist) { return 0; }

int amgx_dist_rhs_buffer(amgx_dist d, double** b, int64_t* n_owned, int64_t* n_ext) {
  if (!d || !d->d) return 1;
  if (b) *b = d->d->bext[0].p;
  if (n_owned) *n_owned = d->d->n(0);
  if (n_ext) *n_ext = d->d->next(0);
  return 0;
}

int amgx_dist_handles(amgx_dist d, amgx_handle* top, amgx_handle* tail) {
  // borrowed views for queries / measurement (amgx_matrix_info, amgx_time_op): one pair per rank object, owned by the
  // communicator; after amgx_comm_destroy they are null handles (every amgx_* call on them returns an error)
  if (!d || !d->d) return 1;
  amgx::Comm* c = d->d->comm;
  if (!d->d->view_top) { d->d->view_top = new amgx_handle_t{d->d->top.get()}; c->handle_views.push_back(d->d->view_top); }
  if (!d->d->view_tail) { d->d->view_tail = new amgx_handle_t{d->d->tail.get()}; c->handle_views.push_back(d->d->view_tail); }
  if (top) *top = d->d->view_top;
  if (tail) *tail = d->d->view_tail;
  return 0;
}

int amgx_dist_apply(amgx_comm cc, const double* const* b, double* const* x, int b_status, int flags) {
  return cguard(cc, [&](amgx::Comm& c) { amgx::dist_apply(c, b, x, b_status, flags); });
}

int amgx_dist_cheb_estimate(amgx_comm cc) {
  return cguard(cc, [&](amgx::Comm& c) { amgx::dist_cheb_estimate(c); });
}

int amgx_dist_time_kernel(amgx_comm cc, int level, int op, int reps, double* avg_ms) {
  return cguard(cc, [&](amgx::Comm& c) {
    using namespace amgx;
    if (c.members.empty() || (c.kind == AMGX_COMM_LOCAL && (int)c.members.size() != c.nranks)) throw Err("amgx_dist_time_kernel: not all ranks have a hierarchy");
    if (reps < 1 || !avg_ms || (op != 8 && op != 9)) throw Err("amgx_dist_time_kernel: bad arguments (op 8: fused Jacobi down kernel, op 9: backward block-hybrid sweep)");
    Dist* d0 = c.members[0];
    if (level < 0 || level >= d0->k) throw Err("amgx_dist_time_kernel: not a rank-partitioned level");
    Handle& h = *d0->top;
    DevLevel& L = h.lev[level];
    if (op == 8 && (!L.paths.jacobi_down() || d0->path != DistPath::JACOBI_FOLDED)) throw Err("amgx_dist_time_kernel: level has no fused pre-smoothing + restriction kernel");
    if (op == 9 && !(d0->path == DistPath::GS_BLOCK_HYBRID && L.paths.hybrid())) throw Err("amgx_dist_time_kernel: level has no block-hybrid Gauss-Seidel sweep");
    std::vector<const double*> bb;
    std::vector<double*> xx;
    for (Dist* d : c.members) {
      if (d->n(0)) launch(fill_kernel, Handle::grid_for(d->n(0)), BLOCK, 0, c.compute, d->n(0), (uint64_t)2, d->bext[0].p);
      bb.push_back(d->bext[0].p); xx.push_back(d->x0.p);
    }
    Handle::ProbeScope probe(h, op);
    double tot = 0.0;
    dist_apply(c, bb.data(), xx.data(), 1, AMGX_DEVICE_PTR | AMGX_NO_GRAPH);        // warm-up (and RCCL's lazy connections)
    h.probe_level = level;
    for (int i = 0; i < reps; ++i) {
      dist_apply(c, bb.data(), xx.data(), 1, AMGX_DEVICE_PTR | AMGX_NO_GRAPH);
      HIPCHK(hipStreamSynchronize(c.compute));
      tot += probe.elapsed_ms();
    }
    *avg_ms = tot / reps;
  });
}

int amgx_dist_pcg(amgx_comm cc, const double* const* b, double* const* x, double tol, int maxit, int use_precond, int flags, double* errs,
                  int32_t* iters) {
  return cguard(cc, [&](amgx::Comm& c) {
    check_dist_solve("amgx_dist_pcg", c, !b || !x || maxit < 0, b, x, flags, " (it holds the residual)");
    amgx::DistKrylov& K = dist_krylov(c);
    const amgx::DistKrylov::Vec xv{x, 0};
    const int it = ((flags & AMGX_PCG_SINGLE_REDUCTION) && use_precond) ? amgx::pcg_sr(K, b, xv, tol, maxit, errs) : amgx::pcg(K, b, xv, tol, maxit, use_precond != 0, errs);
    if (iters) *iters = it;
  });
}

int amgx_dist_gmres(amgx_comm cc, const double* const* b, double* const* x, double tol, int maxit, int restart, int use_precond, int flags,
                    double* errs, int32_t* iters) {
  return cguard(cc, [&](amgx::Comm& c) {
    check_dist_solve("amgx_dist_gmres", c, !b || !x || maxit < 0 || restart < 1, b, x, flags, "");
    const int it = amgx::gmres(dist_krylov(c), b, amgx::DistKrylov::Vec{x, 0}, tol, maxit, restart, use_precond != 0, errs);
    if (iters) *iters = it;
  });
}

// ---- stand-alone halo maps (the DCCMap surface: python_smoothers / tests use it without a hierarchy) -----------------
int amgx_halo_create(amgx_comm cc, const amgx_halo_desc* d, int64_t n_owned, int64_t n_ghost, int32_t bs, int32_t rank, amgx_halo* out) {
  return cguard(cc, [&](amgx::Comm& c) {
    if (!d || !out) throw amgx::Err("amgx_halo_create: null argument");
    if (bs < 1 || bs > 6) throw amgx::Err("amgx_halo_create: block size must be in 1..6");
    auto h = std::make_unique<amgx_halo_t>();
    h->c = &c;
    // world size 1 over RCCL: a rank may list itself as peer (self send / receive) -- used to exercise the wire on one GPU
    h->t.build(*d, n_owned, n_owned + n_ghost, bs, c.nranks, c.nranks > 1 ? (c.kind == AMGX_COMM_RCCL ? c.rank : rank) : -1);
    *out = h.release();
  });
}
int amgx_halo_destroy(amgx_halo h) { delete h; return 0; }

// mode 0: owner -> ghost, overwrite (CO2CU); mode 1: ghost -> owner, add, ghosts zeroed (DIS2CO).
// halos / vecs: one per local rank (RCCL: one); device vectors of (n_owned + n_ghost) * bs entries on the communicator's stream
int amgx_halo_exchange(amgx_comm cc, int n_local, const amgx_halo* halos, double* const* vecs, int mode) {
  return cguard(cc, [&](amgx::Comm& c) {
    if (n_local < 1 || !halos || !vecs) throw amgx::Err("amgx_halo_exchange: bad arguments");
    if (c.kind == AMGX_COMM_RCCL && n_local != 1) throw amgx::Err("amgx_halo_exchange: one rank per process under RCCL");
    if (c.kind == AMGX_COMM_LOCAL && n_local != c.nranks) throw amgx::Err("amgx_halo_exchange: pass all local ranks");
    std::vector<amgx::Comm::Item> it;
    for (int i = 0; i < n_local; ++i) { if (!halos[i] || halos[i]->c != &c || !vecs[i]) throw amgx::Err("amgx_halo_exchange: bad halo / vector"); it.push_back({&halos[i]->t, vecs[i]}); }
    if (mode == 0) c.exchange_end(c.exchange_begin(it));
    else if (mode == 1) c.accumulate(it);
    else throw amgx::Err("amgx_halo_exchange: mode must be 0 or 1");
  });
}

}  // extern "C"
