// MI355X-native AMG apply path: device hierarchy, cycle driver and the C ABI of include/amgx.h.
//
// Host-side structure mirrors the reference's solve layer (not its code):
//   Handle                 <-> AMGMatrix                 (reference src/base/solve/amg_matrix.hpp:14-87)
//   Handle::level_smooth   <-> BaseSmoother / ProxySmoother contract (src/base/smoothers/base_smoother.hpp:68-229)
//   Handle::cycle_v/w/bs   <-> SmoothV / SmoothW / SmoothBS (src/base/solve/amg_matrix.cpp:37-307)
//   Handle::smooth_v_from_level <-> SmoothVFromLevel      (amg_matrix.cpp:310-374)
// Everything between the entry point and the result stays on the GPU; one application = a fixed sequence
// of kernel launches on one HIP stream, captured once per (b, x) pair into a hipGraph and replayed.
#include "../../../include/amgx.h"
#include "kernels.hpp"
#include "multi_kernels.hpp"   // the NV = 2, 4 forms of the product kernels (Handle::product)
#include "cheb_schedule.hpp"   // the Chebyshev recurrence as a schedule of first / step calls
#include "down_plan.hpp"       // DownPlan, the value lists of the fused down kernels, Span, unit_range
#include "knobs.hpp"
#include "launch.hpp"          // Err, HIPCHK, IntList, dispatch, contains, launch
#include "graph_cache.hpp"     // GraphCache
#include "../host/dia.hpp"
#include <dlfcn.h>
#include <algorithm>
#include <array>
#include <chrono>
#include <cmath>
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <tuple>
#include <utility>
#include <vector>

namespace amgx {

// roctx ranges named like the reference's timers (AMGMatrix::SmoothV: "AMGMatrix::Mult", "level 0" .. "level 3", "rest",
// "coarse inv", src/base/solve/amg_matrix.cpp:166-178; "ProlMap::TransferF2C" / "ProlMap::TransferC2F",
// src/base/coarsening/dof_map.cpp:616-630; "GSS3<bs=N>::SmoothRHS", src/base/smoothers/gssmoother.cpp:201,266), so a
// rocprofv3 --marker-trace of the GPU path lines up with an NGSolve trace of the CPU path.  Host-side ranges around the
// enqueue sections; active only with AMGX_ROCTX=1 (libroctx64 is resolved at run time).
struct Roctx {
  int (*push)(const char*) = nullptr;
  int (*pop)() = nullptr;
  static Roctx& get() {
    static Roctx r;
    static bool init = false;
    if (!init) {
      init = true;
      if (std::getenv("AMGX_ROCTX")) {
        void* h = dlopen("libroctx64.so", RTLD_NOW | RTLD_GLOBAL);
        if (!h) h = dlopen("libroctx64.so.4", RTLD_NOW | RTLD_GLOBAL);
        if (!h) h = dlopen("/opt/rocm/lib/libroctx64.so", RTLD_NOW | RTLD_GLOBAL);
        if (h) { r.push = (int (*)(const char*))dlsym(h, "roctxRangePushA"); r.pop = (int (*)())dlsym(h, "roctxRangePop"); }
        if (!r.push || !r.pop) { r.push = nullptr; r.pop = nullptr; }
      }
    }
    return r;
  }
};
struct Range {
  bool on;
  explicit Range(const char* name) : on(Roctx::get().push != nullptr) { if (on) Roctx::get().push(name); }
  explicit Range(const std::string& name) : Range(name.c_str()) {}
  ~Range() { if (on) Roctx::get().pop(); }
  Range(const Range&) = delete;
  Range& operator=(const Range&) = delete;
};
// GSS3<bs>::SmoothRHS of the reference, the marker of a Gauss-Seidel sweep on any number of vectors.  Literals: the launchers build
// no string per call, so the marker costs one test where AMGX_ROCTX is not set.
static const char* gs_range_name(int bs) {
  switch (bs) {
    case 1: return "GSS3<bs=1>::SmoothRHS";
    case 2: return "GSS3<bs=2>::SmoothRHS";
    case 3: return "GSS3<bs=3>::SmoothRHS";
    case 6: return "GSS3<bs=6>::SmoothRHS";
    default: return "GSS3<bs>::SmoothRHS";             // (the sweep kernels are listed for these four)
  }
}
static const char* level_range_name(int l) {          // lev_timers of the reference: levels >= 4 share "rest"
  static const char* n[] = {"level 0", "level 1", "level 2", "level 3", "rest"};
  return n[l < 4 ? l : 4];
}

template <class T>
struct DevBuf {
  T* p = nullptr;
  size_t n = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept { if (this != &o) { release(); p = o.p; n = o.n; o.p = nullptr; o.n = 0; } return *this; }
  ~DevBuf() { release(); }
  void release() { if (p) { (void)hipFree(p); p = nullptr; n = 0; } }
  void alloc(size_t count) {
    release();
    n = count;
    if (count) HIPCHK(hipMalloc((void**)&p, count * sizeof(T)));
  }
  void upload(const T* host, size_t count) {
    alloc(count);
    if (count) HIPCHK(hipMemcpy(p, host, count * sizeof(T), hipMemcpyHostToDevice));
  }
  template <class A> void upload(const std::vector<T, A>& v) { upload(v.data(), v.size()); }
};

enum Fmt : int { FMT_CSRVEC = 0, FMT_SELL = 1, FMT_BSELL = 2, FMT_RB = 4 };     // (3 is reported for windowed SELL, see amgx_matrix_info)

// gathered-vector access of the BSELL kernels (BSellMat::xmode; Knobs::bsell_xmode, same arithmetic in every mode).
// Same box, cfg 3 GS / cfg 5 GS / cfg 5 block-Jacobi applications per second (profiles/r04/gs_experiments.txt):
//   0 (BS 8-byte loads) 281.9 / 160.6 / 193.1    1 (16-byte loads) 277.7 / 160.4 / 189.3    2 (one load + lane exchange) 246.2 / 149.9 / 189.3
// another box: 0 270.4 / 158.5 / 194.1; column indices 2 / 3 / 4 steps ahead (3 / 5 / 4): 261.6 / 154.7 / 193.9, 267.1 / 157.2 / 186.6, 229.5 / 126.7 / 186.3

struct DevMatrix {
  int64_t n_rows = 0, n_cols = 0, nnz = 0;
  int br = 1, bc = 1;
  int fmt = FMT_CSRVEC;
  int lanes = 1;                       // G of the CSR-vector kernels
  // CSR
  DevBuf<int32_t> rowptr, col;
  DevBuf<double> val;
  // SELL-64-pair
  int n_slices = 0;
  int64_t stored = 0;                  // stored entries incl. padding
  int64_t stream_bytes = 0;            // bytes of matrix data one SpMV reads from HBM (values + indices + pointers)
  struct Sell {
    DevBuf<int64_t> slice_ptr;
    DevBuf<int32_t> col32, cbase;
    DevBuf<uint16_t> col16;
    DevBuf<double> val;
    int rowrel = 0, diag_first = 0, wdiag = 0;
    int xcd = 0;                       // workgroup -> rows mapping of the streaming kernels: see SellMat::xcd
    // windowed form (sell_win_spmv_kernel): inside every window of `win` consecutive rows the rows are stored in order
    // of decreasing length (slice padding 1.42 -> 1.08 on Q at cfg 2); rowloc[slot] = row of the slot inside its window
    int win = 0;
    DevBuf<uint16_t> rowloc;
    SellMat view() const { return SellMat{slice_ptr.p, col32.p, col16.p, cbase.p, val.p, rowrel, diag_first, wdiag, xcd}; }
    SellMat view_of(const double* v) const { return SellMat{slice_ptr.p, col32.p, col16.p, cbase.p, v, rowrel, diag_first, wdiag, xcd}; }
    SellMatT<float> view32(const float* v32) const { return SellMatT<float>{slice_ptr.p, col32.p, col16.p, cbase.p, v32, rowrel, diag_first, wdiag, xcd}; }
    // the sweep-only images of a scalar Gauss-Seidel level (DevGS::sell / lower / upper, DevGSB::full / fullLW / lowin) carry their float
    // values here (mat_f32_image); `val` is released where they exist.  An image inside a DevMatrix uses DevMatrix::val32.
    DevBuf<float> val32;
    SellMatT<float> view32() const { return view32(val32.p); }
  } sell;
  struct Rb {                          // rigid-body transfer blocks (kernels.hpp, RbMat): P_ik = w_ik Q(t_ik), or its transpose
    int dim = 0, bf = 0, bc = 0;       // spatial dimension of Q (0: w I), fine / coarse block size
    bool transposed = false;           // rows = coarse vertices (P^T)
    int lanes = 16;
    DevBuf<int32_t> ptr, col;
    DevBuf<double> w, t;
    int64_t nnz = 0;
    RbMat view() const { return RbMat{ptr.p, col.p, w.p, t.p, nnz}; }
  } rb;
  struct BSell {                       // block SELL (kernels.hpp, BSellMat)
    DevBuf<int64_t> slice_ptr;
    DevBuf<int32_t> col;
    DevBuf<double> val;
    BSellMat view(int xmode) const { return BSellMat{slice_ptr.p, col.p, val.p, xmode}; }
    BSellMat view_of(const double* v, int xmode) const { return BSellMat{slice_ptr.p, col.p, v, xmode}; }
    BSellMatT<float> view32(const float* v32, int xmode) const { return BSellMatT<float>{slice_ptr.p, col.p, v32, xmode}; }
  } bsell;
  // single-precision image (A of a Chebyshev level with mat_prec = AMGX_PREC_F32, plain SELL or BSELL only): the
  // value array of the format above rounded to float, same layout, every index array shared.  Built by mat_f32_image
  // (build_level.hpp); read by the smoother passes of Handle::product and by the fused residual + restriction, by nothing else.
  // also A and the BSELL sweep images of a Gauss-Seidel block level (DevLevel::gs32), read by its sweeps and residuals.
  // also the images of a scalar Jacobi level with jacobi_prec = AMGX_JACOBI_PREC_F32 (A, A', Q and the local-window
  // forms; DevLevel::jp32), read by the Jacobi passes of the level.  There the fp64 values of every image but A are released.
  DevBuf<float> val32;
  // The rounded values of A at fp64 width, in the layout of A's format, read by the smoother passes in place of the true ones: under
  // AMGX_GS_F32_WIDE (A/B twin of 5.17; the sweep-only images hold their rounded values in the fp64 array itself), and on a
  // Gauss-Seidel level with float sweep images whose A stayed in block CSR (a small level: no float kernel, no bytes to save, but the
  // same rounded operator in the sweeps and in the residual).  A keeps its true values for amgx_matvec and the Krylov drivers.
  DevBuf<double> val64r;
  bool has32() const { return val32.p != nullptr; }
  int64_t stream_bytes32() const { return stream_bytes - 4 * (int64_t)val32.n; }
  bool empty() const { return n_rows == 0; }
};

struct DevGS {                          // colour-major data for multicolour Gauss-Seidel
  int n_colors = 0;
  // scalar: SELL copy of A in colour-major row order
  std::vector<int> color_slice_ptr;     // [n_colors+1] slice ranges
  int lanes = 1;                        // G of the colour-major SELL-G copy
  DevMatrix::Sell sell;
  // split copies for pre-smoothing from x = 0 (forward sweep needs only lower-colour couplings, the residual after it
  // only higher-colour couplings): one pass over A instead of two
  DevMatrix::Sell lower, upper;
  int n_slices_total = 0;
  bool has_split = false;
  DevBuf<int32_t> rowid;
  // block: colour-major row list over the CSR of A
  std::vector<int> color_row_ptr;       // [n_colors+1]
  DevBuf<int32_t> rowlist;
  // block, preferred: colour-major BSELL copy (bgs_bsell_color_kernel); color_slice_ptr / rowid as in the scalar form
  DevMatrix bcopy;
  bool bsell_ok = false;
  // block levels, pre-smoothing from x = 0: the couplings to lower / to higher colours only (as `lower` / `upper` above)
  DevMatrix blower, bupper;
  bool bsplit = false;
};

struct DevGSB {                         // block-hybrid Gauss-Seidel (gsb_sweep_kernel): blocks of B consecutive rows
  int B = 0, G = 1, TH = 1024;          // rows per block, lanes per row, workgroup size (B * G == TH)
  int n_blocks = 0, n_colors = 0;
  int lowin_maxw = 0;                   // widest slice of `lowin` (entries per lane): <= 5 selects the narrow sweep-from-zero kernel
  // launch-time choices of the sweep, decided once by build_gsb (gsb_set_paths); gsb_sweep and amgx_level_paths read them
  bool narrow = false, mid = false, lw = false;
  // long-row levels: local-window image of `rest` (sell_lw_pre_restrict_kernel, MODE 1) for the fused residual + restriction
  DevMatrix restLW;
  DevBuf<int32_t> lw_cptr, lw_ccol;
  // ... and of `full` for the general sweep (gsb_sweep_kernel<..., LW>): codes instead of columns, see GsbArgs
  DevMatrix::Sell fullLW;
  DevBuf<int32_t> flw_cptr, flw_ccol;
  bool has_fullLW = false;
  int64_t flw_no_window = 0;            // blocks of `fullLW` that keep global 32-bit columns (list over GSB_LW_CAP)
  int full_maxw = 0;                    // widest slice of `full`: <= 11 selects the mid-width general sweep (fewer registers: two 1024-lane
                                        //   workgroups per CU instead of one, so that one block's colour phases hide behind another's loads)
  DevMatrix::Sell full, lowin;          // block-local SELL-G copies (slots colour-sorted inside a block): all entries /
                                        //   only the in-block couplings to LOWER colours (forward sweep from x = 0)
  DevBuf<int32_t> rowid;
  DevBuf<uint8_t> slotcolor;
  DevMatrix rest;                       // natural-order copy of everything `lowin` leaves out, without the diagonal
  DevBuf<double> cvec;                  // 1 / dinv - a_kk: r = c .* x - rest x right after the sweep from zero
  bool has_split = false;
  bool on() const { return B > 0; }
};

// launch-time choices of the block-hybrid sweep (gsb_sweep) and of the multicolour row-list kernel (gs_sweep); amgx_level_paths
// reports the same values
static void gsb_set_paths(const Knobs& K, DevGSB& g) {
  // the sweep from zero over `lowin` takes the narrow kernel (2 entries per lane and pass)
  g.narrow = g.lowin_maxw > 0 && g.lowin_maxw <= 5 && !K.gsb_no_narrow;
  // the general sweep over `full` takes the mid-width kernel (5 entries per lane and pass)
  g.mid = g.G > 1 && g.full_maxw > 0 && g.full_maxw <= 11 && !K.gsb_no_mid;
  // ... and reads its local-window image
  g.lw = g.has_fullLW && g.G > 1;
}
// lanes per block row W of bgs_color_kernel for a colour of `rows` rows on a level with `avg` blocks per row
static int bgs_rowlist_w(double avg, int64_t rows) {
  int W = avg >= 48.0 ? 4 : (avg >= 20.0 ? 2 : 1);
  if (avg >= 32.0 && rows <= 4096) W = 8;      // short colours of long rows: latency, not bandwidth -- spread the row further
  return W;
}

struct DevBGSB {                        // block-hybrid Gauss-Seidel on square-block levels (bgsb_sweep_kernel)
  int BB = 0;                           // block rows per workgroup
  int n_blocks = 0, n_colors = 0;
  DevMatrix off, in, upin;              // BSELL images, every entry of A in exactly one: `in` / `upin` = the in-block couplings to LOWER /
                                        //   HIGHER colours (local block columns, rows sorted by colour inside the block); `off` = everything
                                        //   else incl. the diagonal blocks (global block columns, block-list row order).  A forward sweep
                                        //   walks `in` colour by colour and streams `upin` with the sweep-start values, a backward one the reverse
  DevBuf<int32_t> off_ptr, in_ptr, in_row;   // slice ranges per block / per (block, colour); local block row of every `in` slot (-1: padding)
  DevBuf<int32_t> blk_ptr, blk_rows;         // block rows of every sweep block (runs of consecutive rows, or compact blocks: gs_block_ids)
  // pre-smoothing from x = 0 in ONE pass over A (like DevGSB::lowin / rest): the sweep from zero reads `in` only; afterwards
  // b_k - acc_k = Dmod_k x_k = fac_k A_kk x_k on every swept row, hence r = b - A x = -(R x) with R = A - L_in and the diagonal
  // blocks scaled by (1 - fac_k), stored negated in `rest` (natural order BSELL): r = rest * x
  DevMatrix rest;
  bool has_split = false;
  // block-COLOURED form (amgx_level_desc.gs_block_color, bgsb_sweep_kernel): the sweep blocks listed by block colour; a sweep =
  // one in-place launch per block colour.  `offlo` = the part of `off` a sweep from zero needs: the couplings to swept rows of blocks
  // with a LOWER block colour (the diagonal blocks and the couplings to rows that are never swept multiply zeros there); `rest` then
  // holds -(couplings to higher block colours + `upin`): after the sweep from zero r_k = -sum_{j swept after k} A_kj x_j, so sweep
  // + residual still read A once in total
  bool bc = false;
  int n_bcolors = 0;
  std::vector<int> bc_ptr;              // [n_bcolors + 1] ranges of blk_list
  DevBuf<int32_t> blk_list;
  DevMatrix offlo;
  bool on() const { return BB > 0; }
};

struct DevBGS {                         // block Gauss-Seidel over aggregate blocks (bgs_block_kernel)
  int n_colors = 0;
  int max_m = 0;                        // largest block (scalar dofs)
  std::vector<int> color_ptr;           // [n_colors+1] ranges of the colour-major block list
  DevBuf<int32_t> blocklist, block_ptr, block_rows;
  DevBuf<int64_t> dinv_ptr;
  DevBuf<double> dinv;
  DevBuf<int32_t> rowptr, col;          // CSR of A (the level matrix itself may live in a SELL format)
  DevBuf<double> val;
};
// the instantiation bgs_block_kernel<BS, TH, G> a level's sweep launches, from the blocks per row `avg` of A and the scalar dofs
// max_m of the largest block; bgs_sweep launches it and amgx_level_paths reports it.  G = lanes per scalar row ~ row length / 6;
// TH: one pass over the block's rows where possible (max_m * G <= TH).  The long-row forms (G = 8, 16) are built for 1024 lanes
// only: G = 8 means max_m > 64, i.e. max_m * 8 > 512, so a <512, 8> kernel could never be picked, and G = 16 always took <1024, 16>.
// TH >= max_m holds for every block the set-up admits (max_m <= 256 / G, <= 512 / G or <= BGS_MAX_M = 1024 = the largest TH).
struct BgsShape { int TH, G; };
static BgsShape bgs_block_shape(double avg, int max_m) {
  const int G = avg > 30.0 ? (max_m * 16 <= 1024 ? 16 : 8) : 4;
  const int TH = G != 4 ? 1024 : (max_m * G <= 256 ? 256 : (max_m * G <= 512 ? 512 : 1024));
  return BgsShape{TH, G};
}
// the kernel Handle::product<1, EP> launches on a matrix in the block CSR format (blocks other than 1 x 1, no BSELL / rigid-body image);
// amgx_level_paths reports the same value.  rowlane: bcsr_rowlane_kernel with `width` = W lane groups per block row, chosen from
// the average row length; otherwise bcsrvec_spmv_kernel with `width` = G lanes per block row (DevMatrix::lanes within 2 .. 16).
// Short rectangular rows, i.e. prolongations with <= 4 blocks per row, stay with the lane-per-block kernel (measured), and so
// does every block with a unit dimension.  square_ep: an epilogue that is built for square blocks only (EP_JAC, EP_CHEB).
struct BcsrKernel { bool rowlane; int width; };
static BcsrKernel bcsr_kernel(const DevMatrix& M, bool square_ep) {
  if (M.br >= 2 && M.bc >= 2 && (!square_ep || M.br == M.bc) && (M.br == M.bc || M.nnz >= 6 * M.n_rows)) {
    const double avg = M.n_rows ? (double)M.nnz / (double)M.n_rows : 0.0;
    return BcsrKernel{true, avg >= 48.0 ? 4 : (avg >= 20.0 ? 2 : 1)};
  }
  return BcsrKernel{false, std::min(M.lanes, 16) < 2 ? 2 : std::min(M.lanes, 16)};
}

struct DevRestrict {                    // column-blocked P^T (see restrict_chunk_kernel)
  int n_chunks = 0;
  int64_t n_slots = 0;
  DevBuf<int32_t> chunk_slot, slot_ptr, optr, oidx, dest;     // dest = inverse of oidx (empty: partials stay in slot order)
  DevBuf<double> w, part;
  DevBuf<uint16_t> fi;
  int ept = 4;                          // entries of P per thread of the fused kernels (4 or 6: the fullest chunk decides)
  int max_slots = 0;                    // most slots / entries of P in one chunk (amgx_level_paths reports them)
  int64_t max_entries = 0;
  // compact chunks (cluster_slices): chunk c works on the 64-row slices slice_list[c * spc .. (c + 1) * spc) instead of spc
  // consecutive ones (-1: no slice); empty = consecutive slices
  DevBuf<int32_t> slice_list;
  // box chunks (dia::box_grid): chunk c works on the grid lines of box c, a list of runs (first row, length) that the kernel
  // derives from `box`; lds_doubles = r + max(x_j, products) of the fullest box
  bool boxed = false;
  dia::BoxGrid box = {};
  int64_t box_lds_doubles = 0;
  bool empty() const { return n_chunks == 0; }
  RestrictMat view() const { return RestrictMat{chunk_slot.p, slot_ptr.p, w.p, fi.p, part.p, dest.p}; }
};

// symmetric diagonal image of a scalar Jacobi level's A for the fused down kernel (dia_pre_restrict_kernel; host/dia.hpp):
// replaces the SELL image of A' = A diag(omega Dinv) on that level
struct DevDia {
  int K = 0;                            // upper diagonals (0: the level has no DIA image)
  int xcd = 0;
  int32_t off[DIA_MAX_UPPER] = {};
  DevBuf<double> val;                   // [K * n]
  DevBuf<float> val32;                  // the same values as float (mat_f32_image); `val` is released where it exists
  bool on() const { return K > 0; }
  bool has32() const { return val32.p != nullptr; }
  template <class V>
  DiaMatT<V> view_as(const V* v) const {
    DiaMatT<V> m{v, xcd, {}};
    for (int k = 0; k < DIA_MAX_UPPER; ++k) m.off[k] = off[k];
    return m;
  }
  DiaMat view() const { return view_as<double>(val.p); }
  DiaMatT<float> view32() const { return view_as<float>(val32.p); }
};

struct DevCsr {                         // plain CSR copy for the single-workgroup coarse tail
  DevBuf<int32_t> rowptr, col;
  DevBuf<double> val;
  void upload(const amgx_matrix& A, const double* scaled_vals = nullptr) {
    const int64_t nnz = A.rowptr[A.n_rows];
    std::vector<int32_t> rp(A.n_rows + 1);
    for (int64_t i = 0; i <= A.n_rows; ++i) rp[i] = (int32_t)A.rowptr[i];
    rowptr.upload(rp);
    col.upload(A.col, nnz);
    val.upload(scaled_vals ? scaled_vals : A.val, nnz);
  }
};

// The paths of a level through the cycle.  resolve_paths() turns the presence of the level's images into these values once, when
// amgx_create has built (and possibly released) them; the apply side, the reports and the timers read the values and never probe
// the images again.  The numbers of the first two are the codes amgx_level_paths reports (include/amgx.h, entries 0 and 19).
enum DownPath : int {                   // fused down kernel (pre-smoothing + restriction)
  DOWN_NONE = 0, DOWN_SELL = 1, DOWN_WIN = 2, DOWN_LW = 3, DOWN_DIA = 4,     // Jacobi: A' as SELL / windowed SELL / local window; diagonal image
  DOWN_CHEB = 5,                        // Chebyshev from zero, then residual + restriction
  DOWN_GSB = 6,                         // block-hybrid sweep from zero + residual_restrict_after_zero (internal: entry 0 reports it as 0)
  DOWN_DIA_BOX = 7                      // diagonal image on box chunks (internal: entry 0 reports DOWN_DIA, entry 4 reports 2)
};
enum SweepPath : int {                  // Gauss-Seidel form
  SWEEP_NONE = 0, SWEEP_MC = 1, SWEEP_MC_ROWLIST = 2, SWEEP_MC_BSELL = 3, SWEEP_GSB = 4, SWEEP_BGSB = 5, SWEEP_BGSB_BC = 6, SWEEP_BGS = 7
};
struct LevelPaths {
  int down = DOWN_NONE;
  int sweep = SWEEP_NONE;
  bool plain = true;                    // sm_steps <= 1 && !sm_symm: the smoother is one base step, no ProxySmoother around it
  bool folded = false;                  // the V-cycle runs Q on the way up (see fold_prolongation)
  // the Gauss-Seidel step (Handle::sweep, sweep_from_zero, residual_after_zero read these and never the images' flags)
  bool in_place = true;                 // the sweep updates x in place; otherwise it reads xin and writes xout (SWEEP_GSB, SWEEP_BGSB)
  bool zero_split = false;              // the level has the images for "sweep from zero over the lower couplings, residual from the rest"
  int unit_rows = 0;                    // block rows of one sweep block, the unit of a partial sweep of the hybrid forms (0: the units are colours)
  bool jacobi_down() const { return down == DOWN_SELL || down == DOWN_WIN || down == DOWN_LW || down == DOWN_DIA || down == DOWN_DIA_BOX; }
  bool bgsb() const { return sweep == SWEEP_BGSB || sweep == SWEEP_BGSB_BC; }     // block-hybrid forms: square-block levels,
  bool hybrid() const { return sweep == SWEEP_GSB || bgsb(); }                    //   ... or any level
};

// Part of a Gauss-Seidel sweep: the units [beg, end) (end < 0: up to the last one).  A unit is a sweep block of
// LevelPaths::unit_rows block rows on the hybrid forms and a colour on the multicolour and aggregate-block forms.
struct Units { int beg = 0, end = -1; };

struct DevLevel {
  LevelPaths paths;
  // the fused down launches (down_plan.hpp, Handle::down_launch): through RF -- Jacobi from zero, or the residual after Chebyshev --
  // and through RG, the residual after a block-hybrid sweep (residual_restrict_after_zero)
  DownPlan plan_rf, plan_rg;
  DevCsr tA, tApre, tP, tPT;            // only on tail levels
  DevBuf<int32_t> t_rowlist, t_cptr, t_rowcolor;    // colour-major row list (and the colour of every row) of a Gauss-Seidel tail level
  DevRestrict R;
  DevRestrict RF;                       // chunk-local P^T for sell_pre_restrict_kernel (fused pre-smoothing + restriction)
  int fused_block = 1024;               // workgroup size = rows per chunk of the fused kernel
  DevMatrix A, P, PT;
  DevMatrix Apre;                       // scalar Jacobi levels: A * diag(omega * dinv), see EP_PRE in kernels.hpp
  DevDia dia;                           // ... or, on levels whose A qualifies, its symmetric diagonal image (then Apre stays empty)
  // long-row levels: a second image of A' for the fused down kernel only, with chunk-local 16-bit columns into the sorted list of
  // the distinct columns of every 256-row chunk (sell_lw_pre_restrict_kernel: the gathered vector is staged in LDS)
  DevMatrix ApreLW;
  DevBuf<int32_t> lw_cptr, lw_ccol;
  // the same for the folded prolongation Q (sell_lw_win_spmv_kernel): windowed SELL with window-local 16-bit columns
  DevMatrix QLW;
  DevBuf<int32_t> qlw_cptr, qlw_ccol;
  DevMatrix Q;                          // scalar Jacobi levels of the V-cycle: (I - omega*Dinv*A) P, see fold_prolongation()
  DevBuf<double> dinv;
  // Gauss-Seidel block level with mat_prec = AMGX_PREC_F32 (decided by mat_f32_image): the sweeps and the residual
  // after the sweep from zero read the float images (DevMatrix::val32) of A and of every BSELL image below;
  // gs32_images / gs32_bytes: how many there are and the bytes of their values.  gs32_wide: the AMGX_GS_F32_WIDE twin instead (the
  // fp64 kernels on the rounded values; gs32 stays false)
  bool gs32 = false, gs32_wide = false;
  int gs32_images = 0;
  int64_t gs32_bytes = 0;
  // scalar Jacobi level with jacobi_prec != 0 (decided by mat_f32_image).  jp32: the Jacobi passes read the float
  // images (DevMatrix::val32, DevDia::val32).  jp32_wide: the twin -- the fp64 images hold the rounded values (A: DevMatrix::val64r).
  // jp_mask: the images converted (A, A', A'-LW, DIA, Q, QLW = bits 0 .. 5); jp_bytes: bytes of the converted value arrays;
  // jp_released: fp64 value bytes given back.
  bool jp32 = false, jp32_wide = false;
  int jp_mask = 0;
  int64_t jp_bytes = 0, jp_released = 0;
  // scalar Gauss-Seidel level with mat_prec = AMGX_PREC_F32_SCALAR_GS (decided by mat_f32_image).  sgs32: the sweeps and
  // the residual after the sweep from zero read float images.  sgs32_wide: the AMGX_GS_F32_WIDE twin -- the fp64 images hold the rounded
  // values (A: DevMatrix::val64r).  sgs_mask: the images converted (A, full, fullLW, lowin, rest, restLW, sell, lower, upper = bits
  // 0 .. 8); sgs_bytes: bytes of the converted value arrays; sgs_released: fp64 value bytes given back.
  bool sgs32 = false, sgs32_wide = false;
  int sgs_mask = 0;
  int64_t sgs_bytes = 0, sgs_released = 0;
  DevGS gs;
  DevGSB gsb;
  DevBGSB bgsb;
  DevRestrict RG;                       // chunk-local P^T for the fused residual + restriction after a block-hybrid sweep
  DevBGS bgs;
  int sm_type = AMGX_SM_JACOBI;
  double omega = 0.9;
  int sm_steps = 1, sm_symm = 0;
  int64_t n = 0;                        // block rows (= owned rows of a rank-partitioned level)
  int64_t ncols = 0;                    // block columns of A (>= n: owned + ghost columns)
  int bs = 1;
  int64_t len() const { return n * bs; }
  int64_t ext_len() const { return ncols * bs; }
  DevBuf<double> x, rhs, res, tmp;      // x_level / rhs_level / res_level (amg_matrix.cpp:19-26) + ping-pong buffer
  // AMGX_SM_CHEBY: degree k, interval [lmin, lmax] of Dinv A, coefficients of the recurrence
  //   step 1: d = c0 Dinv r;  step j >= 2: d = c1[j] d + c2[j] Dinv (b - A x);  x += d      (fp64, fixed at create time)
  int cheb_degree = 0, cheb_estimated = 0;
  double cheb_ratio = 10.0, cheb_lmax = 0.0, cheb_lmin = 0.0, cheb_c0 = 0.0;
  double cheb_c1[9] = {}, cheb_c2[9] = {};
  DevBuf<double> d;                     // the update vector of the recurrence
  void cheb_set_interval(double lmax) {
    cheb_lmax = lmax; cheb_lmin = lmax / cheb_ratio;
    const double theta = 0.5 * (cheb_lmax + cheb_lmin), delta = 0.5 * (cheb_lmax - cheb_lmin), sigma = theta / delta;
    cheb_c0 = 1.0 / theta;
    double rho = 1.0 / sigma;
    for (int j = 2; j <= 8; ++j) {
      const double rn = 1.0 / (2.0 * sigma - rho);
      cheb_c1[j] = rn * rho;
      cheb_c2[j] = 2.0 * rn / delta;
      rho = rn;
    }
  }
};

// the SELL image a fused down launch of `mode` reads (lw: its local-window form); the diagonal-image forms read L.dia
static const DevMatrix& down_image(const DevLevel& L, int mode, bool lw) {
  return mode == 2 ? L.A : mode == 1 ? (lw ? L.gsb.restLW : L.gsb.rest) : (lw ? L.ApreLW : L.Apre);
}

// The fused launch of `mode` through R: which image, which kernel instantiation, which chunks.  Everything the launch used to
// re-check in every cycle is checked here, once: a failure means that amgx_create built data that do not fit together, or a shape
// that no kernel is instantiated for, so it throws from amgx_create.  jacobi_form: the DownPath of a MODE 0 launch.
static DownPlan make_down_plan(const DevLevel& L, const DevRestrict& R, int mode, int jacobi_form = DOWN_NONE) {
  static_assert(DOWN_SLICE == WAVE && DOWN_THREADS == SELL_WIN, "down_plan.hpp counts slices of WAVE lanes; a window is a chunk");
  auto need = [&](bool ok, const char* what) { if (!ok) throw Err("fused down pass (MODE " + std::to_string(mode) + "): " + what); };
  const bool compact = R.slice_list.n > 0;
  const bool dia = mode == 0 && (jacobi_form == DOWN_DIA || jacobi_form == DOWN_DIA_BOX);
  const bool lw = mode == 1 ? !L.gsb.restLW.empty() : jacobi_form == DOWN_LW;
  const DevMatrix& M = down_image(L, mode, lw);
  need(dia || M.fmt == FMT_SELL, "the image is not in a SELL format");
  DownPlan p;
  p.on = true; p.mode = mode; p.ept = R.ept; p.n_chunks = R.n_chunks;
  p.family = dia ? (jacobi_form == DOWN_DIA ? DOWN_FAM_DIA : DOWN_FAM_DIA_BOX) : lw ? DOWN_FAM_LW : M.sell.win ? DOWN_FAM_WIN : DOWN_FAM_SELL;
  p.diags = dia ? L.dia.K : 0; p.lanes = dia ? 1 : M.lanes; p.f32 = ((mode == 2 || mode == 1) && M.has32()) || (mode == 0 && (dia ? L.dia.has32() : M.has32()));
  // (RG and the local-window chunks are always built for DOWN_THREADS lanes; the other builders leave their choice in fused_block)
  p.threads = (mode == 1 || lw) ? DOWN_THREADS : L.fused_block;
  p.unit_rows = down_rows_per_chunk(p.threads, p.lanes);
  p.splittable = down_splittable(p.family, compact);
  // ---- a kernel is instantiated for the shape
  need(p.family == DOWN_FAM_SELL && mode == 0 && p.lanes == 1 ? contains(DownSizes{}, p.threads) : p.threads == DOWN_THREADS, "no kernel for this workgroup size");
  switch (p.family) {
    case DOWN_FAM_SELL:
      if (p.lanes == 1) need(contains(DownEpt{}, p.ept), "no one-lane sell kernel for this EPT");
      else need(mode != 1 && contains(DownSellLanes{}, p.lanes) && p.ept == DOWN_MULTI_EPT && !compact, "no multi-lane sell kernel for this shape");
      break;
    case DOWN_FAM_WIN: need(mode != 2 && p.lanes == 1 && M.sell.win == SELL_WIN && contains(DownEpt{}, p.ept) && !compact, "no windowed kernel for this shape"); break;
    case DOWN_FAM_LW: need(mode != 2 && contains(DownLwLanes{}, p.lanes) && contains(DownLwEpt{}, p.ept) && !compact, "no local-window kernel for this shape"); break;
    case DOWN_FAM_DIA: need(contains(DiaDiags{}, p.diags) && contains(DownEpt{}, p.ept), "no diagonal-image kernel for this shape"); break;
    default: need(contains(DiaBoxDiags{}, p.diags) && !compact, "no box-chunk kernel for this number of diagonals"); break;     // (it loops over any EPT)
  }
  // ---- the chunks of R are the chunks the kernel forms
  const int64_t rows = R.box.box_rows();
  if (p.family == DOWN_FAM_DIA_BOX)
    need(R.boxed && (int64_t)R.box.nx * R.box.ny * R.box.nz == L.n && rows <= dia::BOX_MAX_ROWS && R.box_lds_doubles >= 2 * rows &&
         R.box_lds_doubles >= rows + R.max_entries && R.box_lds_doubles <= DIA_BOX_LDS_DOUBLES, "box / chunk mismatch");
  p.lds_bytes = (size_t)R.box_lds_doubles * sizeof(double);     // (0 unless the chunks are boxes)
  if (p.family == DOWN_FAM_DIA_BOX) { p.box_rows = rows; p.max_entries = R.max_entries; }     // (what down_nv_dia_lds_bytes sizes the NV launch from)
  const int64_t expected = p.family == DOWN_FAM_DIA_BOX ? down_expected_chunks(p.family, R.box.n_boxes(), p.threads, p.lanes)
                           : compact                    ? (int64_t)(R.slice_list.n / down_slices_per_chunk(p.threads))
                                                        : down_expected_chunks(p.family, dia ? L.n : M.n_slices, p.threads, p.lanes);
  need(expected == R.n_chunks, "chunk / slice mismatch");
  if (p.family == DOWN_FAM_LW) {           // the longest column list of a chunk (what down_nv_lw_lds_bytes sizes the NV launch from)
    const DevBuf<int32_t>& cp = mode == 1 ? L.gsb.lw_cptr : L.lw_cptr;
    need((int64_t)cp.n >= (int64_t)R.n_chunks + 1, "chunk / column-list mismatch");
    std::vector<int32_t> h((size_t)R.n_chunks + 1);
    HIPCHK(hipMemcpy(h.data(), cp.p, h.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    for (size_t c = 0; c + 1 < h.size(); ++c) p.lw_max_list = std::max(p.lw_max_list, (int)(h[c + 1] - h[c]));
    need(p.lw_max_list <= LW_CAP, "a column list beyond the window capacity");
  }
  return p;
}

// The ONLY place where image presence becomes a path -- and a path a launch plan.  Precedence of the down kernels: local window
// before diagonal image before SELL; of the sweeps: bgsb before gsb before multicolour.  Conditions on call-time arguments (the part
// of a split level, the fold flag, skip_rsum) stay with the callers.
static int sweep_path(const DevLevel& L) {
  if (L.sm_type == AMGX_SM_BGS) return SWEEP_BGS;
  if (L.sm_type != AMGX_SM_GS) return SWEEP_NONE;
  if (L.bgsb.on()) return L.bgsb.bc ? SWEEP_BGSB_BC : SWEEP_BGSB;
  if (L.gsb.on()) return SWEEP_GSB;
  if (L.gs.n_colors > 0) return L.bs == 1 ? SWEEP_MC : (L.gs.bsell_ok ? SWEEP_MC_BSELL : SWEEP_MC_ROWLIST);
  return SWEEP_NONE;
}
static void resolve_paths(DevLevel& L) {
  LevelPaths p;
  p.plain = L.sm_steps <= 1 && !L.sm_symm;
  // (a level without rows -- a rank that owns nothing -- is trivially folded: every kernel on it is a no-op)
  p.folded = p.plain && L.sm_type == AMGX_SM_JACOBI && (L.n == 0 || (!L.Q.empty() && (L.bs > 1 || !L.Apre.empty() || L.dia.on())));
  p.sweep = sweep_path(L);
  p.in_place = p.sweep != SWEEP_GSB && p.sweep != SWEEP_BGSB;
  p.zero_split = p.bgsb() ? L.bgsb.has_split : p.sweep == SWEEP_GSB ? L.gsb.has_split : p.sweep == SWEEP_MC ? L.gs.has_split : p.sweep == SWEEP_MC_BSELL && L.gs.bsplit;
  p.unit_rows = p.bgsb() ? L.bgsb.BB : p.sweep == SWEEP_GSB ? L.gsb.B : 0;
  if (p.plain && L.sm_type == AMGX_SM_JACOBI && !L.RF.empty())
    p.down = !L.ApreLW.empty() ? DOWN_LW : L.dia.on() ? (L.RF.boxed ? DOWN_DIA_BOX : DOWN_DIA) : L.Apre.sell.win ? DOWN_WIN : DOWN_SELL;
  else if (p.plain && L.sm_type == AMGX_SM_CHEBY && !L.RF.empty()) p.down = DOWN_CHEB;
  else if (p.plain && p.sweep == SWEEP_GSB && L.gsb.has_split && !L.RG.empty()) p.down = DOWN_GSB;
  L.paths = p;
  L.plan_rf = p.jacobi_down() ? make_down_plan(L, L.RF, 0, p.down) : p.down == DOWN_CHEB ? make_down_plan(L, L.RF, 2) : DownPlan();
  // (residual_restrict_after_zero also serves the rank-partitioned driver, whatever the cycle's own down path is)
  L.plan_rg = (L.gsb.on() && L.gsb.has_split && !L.RG.empty()) ? make_down_plan(L, L.RG, 1) : DownPlan();
}

// ---------------------------------------------------------------------------------------------------
// host-side format construction
// ---------------------------------------------------------------------------------------------------

// vectors whose elements are NOT zeroed on resize: the SELL builders write every slot of these arrays themselves, and a serial
// memset of 2.4 GB per image was a third of a second of amgx_create at cfg 2
template <class T>
struct NoInitAlloc : std::allocator<T> {
  template <class U> struct rebind { using other = NoInitAlloc<U>; };
  NoInitAlloc() = default;
  template <class U> NoInitAlloc(const NoInitAlloc<U>&) {}
  template <class U, class... Args> void construct(U* p, Args&&... args) { if constexpr (sizeof...(Args) > 0) ::new ((void*)p) U(std::forward<Args>(args)...); else ::new ((void*)p) U; }
};
template <class T> using RawVec = std::vector<T, NoInitAlloc<T>>;

// AMGX_SETUP_LOG=1: wall-clock time of the stages of amgx_create on stderr
struct SetupClock {
  bool on;
  explicit SetupClock(const Knobs& K) : on(K.setup_log) {}
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  void lap(const char* what, int level = -1) {
    if (!on) return;
    const auto t1 = std::chrono::steady_clock::now();
    std::fprintf(stderr, "[amgx_create] %-42s level %2d  %8.1f ms\n", what, level, std::chrono::duration<double, std::milli>(t1 - t0).count());
    t0 = t1;
  }
};

// Host threads for the format builders of amgx_create (cold path, but 10^8 entries at cfg 2: serial loops were 7.5 s of
// "upload"): contiguous index ranges, one per thread; f(begin, end, thread).  AMGX_SETUP_THREADS overrides the count, which is
// fixed at its first use in the process.
static int setup_threads() {
  static const int T = Knobs::from_env().setup_threads;
  return T;
}
template <class F>
static void par_for(int64_t n, F&& f, int64_t min_per_thread = 4096) {
  const int T = (int)std::max<int64_t>(1, std::min<int64_t>(setup_threads(), n / std::max<int64_t>(1, min_per_thread)));
  if (T <= 1) { f((int64_t)0, n, 0); return; }
  std::vector<std::thread> th;
  std::exception_ptr err = nullptr;
  std::vector<std::exception_ptr> errs(T);
  for (int t = 0; t < T; ++t)
    th.emplace_back([&, t] {
      try { f(n * t / T, n * (t + 1) / T, t); } catch (...) { errs[t] = std::current_exception(); }
    });
  for (auto& q : th) q.join();
  for (auto& e : errs) if (e) std::rethrow_exception(e);
}

// The images of one level (A, P / P^T, smoother data, A', Q) are independent of each other: they are built by concurrent host
// tasks, so the serial pieces of one builder (prefix sums, allocations, the host-to-device copies) overlap with the threaded
// loops of the others.  AMGX_SETUP_SERIAL=1 runs them one after the other.
struct SetupTasks {
  int device;
  bool serial, log;
  std::vector<std::thread> th;
  std::vector<std::exception_ptr> errs;
  std::mutex mu;
  SetupTasks(int dev, const Knobs& K) : device(dev), serial(K.setup_serial), log(K.setup_log) {}
  ~SetupTasks() { for (auto& t : th) if (t.joinable()) t.join(); }
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  template <class F>
  void timed(F& f, const char* name) {
    if (!log) { f(); return; }
    const auto a = std::chrono::steady_clock::now();
    f();
    const auto b = std::chrono::steady_clock::now();
    std::fprintf(stderr, "[amgx_create]   task %-28s %8.1f .. %8.1f ms\n", name, std::chrono::duration<double, std::milli>(a - t0).count(),
                 std::chrono::duration<double, std::milli>(b - t0).count());
  }
  template <class F>
  void run(F f, const char* name = "") {
    if (serial) { timed(f, name); return; }
    th.emplace_back([this, f, name]() mutable {
      try { HIPCHK(hipSetDevice(device)); timed(f, name); }
      catch (...) { std::lock_guard<std::mutex> g(mu); errs.push_back(std::current_exception()); }
    });
  }
  void wait() {
    for (auto& t : th) if (t.joinable()) t.join();
    th.clear();
    if (!errs.empty()) { auto e = errs.front(); errs.clear(); std::rethrow_exception(e); }
  }
};

template <class T>
static void par_assign(RawVec<T>& v, size_t n, T value) {      // resize without the serial value-initialisation, fill on all threads
  v.resize(n);
  T* p = v.data();
  par_for((int64_t)n, [&](int64_t a, int64_t b, int) { std::fill(p + a, p + b, value); }, 1 << 20);
}

// lanes per row of the CSR-vector kernels: the widest group that still keeps >= 80 % of its lanes busy
// (a row of length L costs ceil(L/G) steps of G lanes), else the most efficient one
static int pick_lanes(double avg_len) {
  if (avg_len <= 2.0) return 2;
  int best = 2;
  double best_eff = 0.0;
  for (int g = 64; g >= 2; g >>= 1) {
    const double steps = std::ceil(avg_len / g);
    const double eff = avg_len / (steps * g);
    if (eff >= 0.8) return g;
    if (eff > best_eff) { best_eff = eff; best = g; }
  }
  return best;
}

// Long rows (coarse levels of a reference-shaped hierarchy: 50-100 entries per row, ragged): with one thread per row the 64
// lanes of a wave gather entry k of 64 DIFFERENT rows per step -- 64 unrelated cache lines, the kernel is bound by the
// address path (0.45 T gathers/s measured at the 1.24 M-row level of cfg 2, 4.5 TB/s) -- while G lanes per row walk G
// consecutive (ascending, hence neighbouring) columns of ONE row.  Lanes per row for rows of this average length:
static int sell_long_row_lanes(const Knobs& K, double avg) {
  // measured at that level (same box, 1 / 2 / 4 / 8 lanes): 193 / 176 / 188 / 204 us -- no win, the default stays one lane
  return avg >= 24.0 ? K.sell_long_row_lanes : 1;
}

// SELL-64-pair image of the rows `rows[0..m)` of a scalar CSR matrix (row id < 0 => empty padding row).
// Element (lane, j) of a slice of width w sits at  base + (j/2)*128 + lane*2 + (j&1)  for j < 2*(w/2)
// and at  base + (w-1)*64 + lane  for the odd trailing column.  Padding: value 0, column = a valid index.
// Column indices are stored as 32-bit values and, for every slice where it is possible, additionally as
// 16-bit deltas  col = (rowrel ? row : 0) + cbase[column] + d  (see kernels.hpp, SellMat).
struct HostSell {
  std::vector<int64_t> slice_ptr;
  RawVec<int32_t> col32;
  std::vector<int32_t> cbase;
  RawVec<uint16_t> col16;
  RawVec<double> val;
  int64_t n_comp_slices = 0, stream_bytes = 0;
  int rowrel = 0, diag_first = 0;
};

// G = lanes per row (1, 2, 4, 8, 16).  G == 1: one thread per row, slices of 64 rows, odd widths allowed.
// G > 1 ("SELL-G"): slices of 64/G rows; entry e of a row belongs to lane g = (e/2) % G of the row's lane
// group at step p = (e/2) / G, so every step of a wave still reads one contiguous 1 KiB + 512 B (or 256 B) line
// set; the G partial sums are combined by a wave shuffle reduction in the kernel.
static int64_t sell_stored(const amgx_matrix& A, int G) {
  const int R = WAVE / G;
  const int64_t ns = (A.n_rows + R - 1) / R;
  std::vector<int64_t> part(setup_threads(), 0);
  par_for(ns, [&](int64_t s0, int64_t s1, int t) {
    int64_t stored = 0;
    for (int64_t s = s0; s < s1; ++s) {
      int mx = 0;
      for (int64_t r = s * R; r < std::min<int64_t>(A.n_rows, (s + 1) * R); ++r) mx = std::max<int>(mx, (int)(A.rowptr[r + 1] - A.rowptr[r]));
      const int w = (G == 1) ? mx : 2 * (((mx + 1) / 2 + G - 1) / G);
      stored += (int64_t)w * WAVE;
    }
    part[t] += stored;
  });
  int64_t stored = 0;
  for (int64_t v : part) stored += v;
  return stored;
}

// no16 (optional, per row of A): slices holding such a row keep the 32-bit column encoding
static void build_sell(const amgx_matrix& A, const int32_t* rows, int64_t m, bool rowrel, int G, HostSell& S, bool want_diag_first = false,
                       const std::vector<char>* no16 = nullptr) {
  const int R = WAVE / G;
  const int64_t ns = (m + R - 1) / R;
  S.rowrel = rowrel ? 1 : 0;
  // diagonal-first entry order (one thread per row, square matrix, every row has its diagonal stored): the Jacobi
  // epilogues then get the own-row value of the gathered vector from entry 0 instead of a second streaming read
  std::vector<int32_t> dpos;
  bool diag_first = want_diag_first && G == 1 && !rows && A.n_rows <= A.n_cols;
  if (diag_first) {
    dpos.assign(A.n_rows, -1);
    std::vector<char> bad(setup_threads(), 0);
    par_for(A.n_rows, [&](int64_t i0, int64_t i1, int t) {
      for (int64_t i = i0; i < i1; ++i) {
        for (int64_t k = A.rowptr[i]; k < A.rowptr[i + 1]; ++k) if (A.col[k] == i) { dpos[i] = (int32_t)(k - A.rowptr[i]); break; }
        if (dpos[i] < 0) { bad[t] = 1; break; }
      }
    });
    for (char b : bad) if (b) diag_first = false;
  }
  S.diag_first = diag_first ? 1 : 0;
  // CSR position (relative to the row start) of entry e in the device order
  auto src = [&](int64_t r, int e) -> int { if (!diag_first) return e; const int dp = dpos[r]; return e == 0 ? dp : (e <= dp ? e - 1 : e); };
  S.slice_ptr.assign(ns + 1, 0);
  auto row_of = [&](int64_t q) -> int64_t { return (q < m) ? (rows ? rows[q] : q) : -1; };
  par_for(ns, [&](int64_t s0, int64_t s1, int) {
    for (int64_t s = s0; s < s1; ++s) {
      int mx = 0;
      for (int r = 0; r < R; ++r) {
        const int64_t rr = row_of(s * R + r);
        if (rr < 0) continue;
        mx = std::max<int>(mx, (int)(A.rowptr[rr + 1] - A.rowptr[rr]));
      }
      const int w = (G == 1) ? mx : 2 * (((mx + 1) / 2 + G - 1) / G);
      S.slice_ptr[s + 1] = (int64_t)w * WAVE;            // widths first, offsets by the prefix sum below
    }
  });
  for (int64_t s = 0; s < ns; ++s) S.slice_ptr[s + 1] += S.slice_ptr[s];
  const int64_t stored = S.slice_ptr[ns];
  S.col32.resize(stored);            // (every slot of col32 / col16 / val is written by the fill pass below)
  S.col16.resize(stored);
  S.cbase.assign(stored / WAVE, 0);
  S.val.resize(stored);
  S.n_comp_slices = 0;
  S.stream_bytes = 8 * (ns + 1);
  std::vector<int64_t> t_comp(setup_threads(), 0), t_bytes(setup_threads(), 0);
  std::vector<uint8_t> comp_flag((size_t)ns, 0);           // (the flag goes into bit 0 of slice_ptr[s] after all slices are filled)
  par_for(ns, [&](int64_t sl0, int64_t sl1, int tid) {
  for (int64_t s = sl0; s < sl1; ++s) {
    const int64_t base = S.slice_ptr[s];
    const int w = (int)((S.slice_ptr[s + 1] - base) / WAVE);
    const int wp = w & ~1;
    auto off = [&](int l, int j) { return (j < wp) ? base + (int64_t)(j >> 1) * (2 * WAVE) + l * 2 + (j & 1) : base + (int64_t)(w - 1) * WAVE + l; };
    // (lane l, column j) -> entry index within the lane's row
    auto entry = [&](int l, int j) { return (G == 1) ? j : 2 * ((j >> 1) * G + (l % G)) + (j & 1); };
    bool comp = true;
    if (no16)
      for (int r = 0; r < R; ++r) { const int64_t rr = row_of(s * R + r); if (rr >= 0 && (*no16)[rr]) comp = false; }
    for (int j = 0; j < w; ++j) {
      // pass 1: real entries -> 32-bit columns, column base for the 16-bit form
      int64_t cb = INT64_MAX;
      for (int l = 0; l < WAVE; ++l) {
        const int64_t r = row_of(s * R + l / G);
        if (r < 0) continue;
        const int64_t rb = A.rowptr[r];
        const int len = (int)(A.rowptr[r + 1] - rb);
        const int e = entry(l, j);
        if (e < len) {
          const int64_t o = off(l, j);
          const int64_t ks = rb + src(r, e);
          S.col32[o] = A.col[ks];
          S.val[o] = A.val[ks];
          cb = std::min<int64_t>(cb, (int64_t)A.col[ks] - (rowrel ? r : 0));
        }
      }
      if (cb == INT64_MAX) cb = 0;
      if (cb < INT32_MIN / 2 || cb > INT32_MAX / 2) comp = false;
      S.cbase[base / WAVE + j] = (int32_t)cb;
      // pass 2: deltas and padding
      for (int l = 0; l < WAVE; ++l) {
        const int64_t q = s * R + l / G;
        const int64_t r = row_of(q);
        const int64_t o = off(l, j);
        const int64_t rb = r >= 0 ? A.rowptr[r] : 0;
        const int len = r >= 0 ? (int)(A.rowptr[r + 1] - rb) : 0;
        const int e = entry(l, j);
        // the row id the kernel will use for this lane: plain SELL = position, colour-major = rowid (lanes with r < 0 exit early)
        const int64_t rk = rows ? r : q;
        const int64_t rr = rowrel ? rk : 0;
        if (e < len) {
          const int64_t d = (int64_t)A.col[rb + src(r, e)] - rr - cb;
          if (d < 0 || d > 65535) comp = false; else S.col16[o] = (uint16_t)d;
        } else {
          // padding (value 0): any valid column; prefer one reachable in both encodings
          const int32_t padcol = (r >= 0 && len) ? A.col[rb] : 0;
          S.col32[o] = padcol;
          S.val[o] = 0.0;
          if (rows && r < 0) { S.col16[o] = 0; continue; }      // lane never executes
          int64_t d = (int64_t)padcol - rr - cb;
          if (d < 0 || d > 65535) {
            d = std::max<int64_t>(0, -(rr + cb));                 // smallest delta that gives a column >= 0
            if (d > 65535 || rr + cb + d >= A.n_cols) comp = false;
          }
          if (comp) S.col16[o] = (uint16_t)d;
        }
      }
    }
    if (comp && w > 0) { comp_flag[s] = 1; t_comp[tid]++; t_bytes[tid] += (int64_t)w * WAVE * 10 + 4 * w; }
    else t_bytes[tid] += (int64_t)w * WAVE * 12;
  }
  }, 64);
  for (int64_t s = 0; s < ns; ++s) if (comp_flag[s]) S.slice_ptr[s] |= 1;
  for (int64_t v : t_comp) S.n_comp_slices += v;
  for (int64_t v : t_bytes) S.stream_bytes += v;
}

// G == 1, diagonal-first SELL: overwrite the diagonal slot (entry 0) of every row (see SellMat::wdiag)
static void patch_sell_diag(HostSell& S, int64_t n_rows, const double* dval) {
  const int64_t ns = (int64_t)S.slice_ptr.size() - 1;
  par_for(ns, [&](int64_t s0, int64_t s1, int) {
    for (int64_t s = s0; s < s1; ++s) {
      const int64_t base = S.slice_ptr[s] & ~(int64_t)63;
      const int w = (int)(((S.slice_ptr[s + 1] & ~(int64_t)63) - base) / WAVE);
      if (w == 0) continue;
      for (int l = 0; l < WAVE; ++l) {
        const int64_t row = s * WAVE + l;
        if (row >= n_rows) break;
        S.val[w >= 2 ? base + l * 2 : base + l] = dval[row];
      }
    }
  }, 64);
}

static void upload_sell(const HostSell& S, DevMatrix::Sell& D) {
  const int64_t ns = (int64_t)S.slice_ptr.size() - 1;
  D.rowrel = S.rowrel;
  D.diag_first = S.diag_first;
  D.slice_ptr.upload(S.slice_ptr);
  D.val.upload(S.val);
  if (S.n_comp_slices < ns) D.col32.upload(S.col32);               // only read by 32-bit slices
  if (S.n_comp_slices > 0) {
    D.col16.upload(S.col16);
    // slack behind the last slice: gsb_sweep_kernel reads the column bases of a slice as one unconditional group of 2*GSB_WP + 1
    std::vector<int32_t> cb(S.cbase);
    cb.resize(cb.size() + 32, 0);
    D.cbase.upload(cb);
  }
}

// block SELL image of a square-block matrix (see kernels.hpp BSellMat); returns false if the padding would exceed `max_pad`
// rows (optional): the block rows in storage order (-1 = padding slot), m of them; default = natural order
static bool build_bsell(const amgx_matrix& A, DevMatrix& D, double max_pad, const int32_t* rows = nullptr, int64_t m = -1) {
  const int bs = A.br;
  const int RB = WAVE / bs;
  const int64_t n = rows ? m : A.n_rows;
  const int64_t ns = (n + RB - 1) / RB;
  auto row_of = [&](int64_t q) -> int64_t { return q < n ? (rows ? rows[q] : q) : -1; };
  std::vector<int64_t> sp(ns + 1, 0);
  par_for(ns, [&](int64_t s0, int64_t s1, int) {
    for (int64_t s = s0; s < s1; ++s) {
      int w = 0;
      for (int64_t q = s * RB; q < std::min<int64_t>(n, (s + 1) * RB); ++q) { const int64_t r = row_of(q); if (r >= 0) w = std::max<int>(w, (int)(A.rowptr[r + 1] - A.rowptr[r])); }
      sp[s + 1] = w;
    }
  }, 64);
  for (int64_t s = 0; s < ns; ++s) sp[s + 1] += sp[s];
  const int64_t steps = sp[ns], nnz = A.rowptr[A.n_rows];
  if (nnz == 0 || (double)steps * RB > max_pad * (double)nnz) return false;
  RawVec<int32_t> col;
  RawVec<double> val;
  par_assign(col, (size_t)steps * RB, (int32_t)0);
  par_assign(val, (size_t)steps * bs * WAVE, 0.0);
  par_for(ns, [&](int64_t s0, int64_t s1, int) {
    for (int64_t s = s0; s < s1; ++s) {
      const int w = (int)(sp[s + 1] - sp[s]);
      for (int rb = 0; rb < RB; ++rb) {
        const int64_t r = row_of(s * RB + rb);
        const int64_t rbeg = r >= 0 ? A.rowptr[r] : 0;
        const int len = r >= 0 ? (int)(A.rowptr[r + 1] - rbeg) : 0;
        for (int k = 0; k < w; ++k) {
          const int64_t kk = sp[s] + k;
          col[kk * RB + rb] = k < len ? A.col[rbeg + k] : (int32_t)std::min<int64_t>(std::max<int64_t>(r, 0), A.n_rows - 1);   // padding: a valid block column
          if (k >= len) continue;
          const double* b = A.val + (rbeg + k) * bs * bs;
          double* vk = val.data() + kk * (bs * WAVE);
          for (int rr = 0; rr < bs; ++rr) {
            const int lane = rb * bs + rr;
            for (int c = 0; c < bs; ++c) {
              const int cp = c / 2;
              if ((bs & 1) && c == bs - 1) vk[(bs / 2) * (2 * WAVE) + lane] = b[rr * bs + c];
              else vk[cp * (2 * WAVE) + lane * 2 + (c & 1)] = b[rr * bs + c];
            }
          }
        }
      }
    }
  }, 16);
  D.fmt = FMT_BSELL;
  D.n_slices = (int)ns;
  D.stored = steps * RB;
  D.stream_bytes = steps * ((int64_t)bs * WAVE * 8 + RB * 4) + 8 * (ns + 1);
  D.bsell.slice_ptr.upload(sp); D.bsell.col.upload(col); D.bsell.val.upload(val);
  return true;
}

// Rigid-body structure of a transfer matrix (see RbMat): every block of P (bf x bc) must be w Q(t), every block of P^T (bc x bf)
// its transpose.  Returns false (and leaves D untouched) if any block deviates: the general block formats take over.
static bool try_build_rb(const Knobs& K, const amgx_matrix& M, bool transposed, DevMatrix& D) {
  if (K.no_rb_transfer) return false;
  const int bf = transposed ? M.bc : M.br, bc = transposed ? M.br : M.bc;
  int dim;
  if (bc == 6 && (bf == 3 || bf == 6)) dim = 3;
  else if (bc == 3 && (bf == 2 || bf == 3)) dim = 2;
  else if (bc == 2 && bf == 2) dim = 0;
  else return false;
  const int64_t nnz = M.rowptr[M.n_rows];
  if (nnz == 0 || nnz >= I32_MAX) return false;
  std::vector<double> w((size_t)nnz), t((size_t)std::max(1, dim) * nnz, 0.0);
  std::vector<char> bad(setup_threads(), 0);
  const int br = M.br, bcm = M.bc;
  par_for(nnz, [&](int64_t k0, int64_t k1, int tid) {
    for (int64_t k = k0; k < k1; ++k) {
      const double* b = M.val + k * br * bcm;
      // entry (r of the fine block row, c of the coarse block column) of the un-transposed block
      auto at = [&](int r, int c) { return transposed ? b[c * bcm + r] : b[r * bcm + c]; };
      const double wk = at(0, 0);
      double tt[3] = {0.0, 0.0, 0.0};
      double ex[6][6];
      for (int r = 0; r < bf; ++r) for (int c = 0; c < bc; ++c) ex[r][c] = 0.0;
      const int nd = dim == 0 ? bf : dim;
      for (int r = 0; r < nd; ++r) ex[r][r] = wk;
      for (int r = nd; r < bf; ++r) ex[r][r] = wk;
      if (dim == 3) {
        if (wk != 0.0) { tt[0] = at(1, 5) / wk; tt[1] = at(2, 3) / wk; tt[2] = at(0, 4) / wk; }
        ex[0][4] = wk * tt[2]; ex[0][5] = -wk * tt[1];
        ex[1][3] = -wk * tt[2]; ex[1][5] = wk * tt[0];
        ex[2][3] = wk * tt[1]; ex[2][4] = -wk * tt[0];
      } else if (dim == 2) {
        if (wk != 0.0) { tt[0] = at(1, 2) / wk; tt[1] = -at(0, 2) / wk; }
        ex[0][2] = -wk * tt[1]; ex[1][2] = wk * tt[0];
      }
      const double tol = 1e-13 * (std::fabs(wk) * (1.0 + std::fabs(tt[0]) + std::fabs(tt[1]) + std::fabs(tt[2])));
      for (int r = 0; r < bf; ++r)
        for (int c = 0; c < bc; ++c)
          if (!(std::fabs(at(r, c) - ex[r][c]) <= tol)) { bad[tid] = 1; return; }
      w[k] = wk;
      for (int q = 0; q < dim; ++q) t[(size_t)q * nnz + k] = tt[q];
    }
  }, 1 << 12);
  for (char c : bad) if (c) return false;
  std::vector<int32_t> rp((size_t)M.n_rows + 1);
  for (int64_t i = 0; i <= M.n_rows; ++i) rp[i] = (int32_t)M.rowptr[i];
  D.fmt = FMT_RB;
  D.rb.dim = dim; D.rb.bf = bf; D.rb.bc = bc; D.rb.transposed = transposed; D.rb.nnz = nnz;
  D.rb.ptr.upload(rp); D.rb.col.upload(M.col, (size_t)nnz); D.rb.w.upload(w); D.rb.t.upload(t);
  D.stored = nnz;
  D.stream_bytes = nnz * (4 + 8 + 8 * (int64_t)dim) + 4 * (M.n_rows + 1);
  return true;
}

static void check_matrix(const amgx_matrix& A, const char* what) {
  if (A.n_rows < 0 || A.n_cols < 0 || !A.rowptr) throw Err(std::string(what) + ": invalid matrix descriptor");
  if (A.br < 1 || A.br > 6 || A.bc < 1 || A.bc > 6) throw Err(std::string(what) + ": block sizes must be in 1..6");
  const int64_t nnz = A.rowptr[A.n_rows];
  if (nnz > 0 && (!A.col || !A.val)) throw Err(std::string(what) + ": col / val missing");
  if (nnz >= I32_MAX) throw Err(std::string(what) + ": more than 2^31-1 stored blocks are not supported on the device");
  if (A.n_cols >= I32_MAX / 8) throw Err(std::string(what) + ": too many columns for int32 indices");
  par_for(A.n_rows, [&](int64_t i0, int64_t i1, int) {
    for (int64_t i = i0; i < i1; ++i)
      if (A.rowptr[i + 1] < A.rowptr[i]) throw Err(std::string(what) + ": rowptr is not monotone");
  });
  par_for(nnz, [&](int64_t k0, int64_t k1, int) {
    for (int64_t k = k0; k < k1; ++k)
      if (A.col[k] < 0 || A.col[k] >= A.n_cols) throw Err(std::string(what) + ": column index out of range");
  }, 1 << 16);
}

// rb_mode: 1 = A is a prolongation, 2 = its transpose: block matrices are first tried in the rigid-body form (try_build_rb)
static void upload_matrix(const Knobs& K, const amgx_matrix& A, DevMatrix& D, const char* what, bool allow_sell = true, bool rowrel_ok = false, bool keep_csr = false,
                          double max_pad = 1.35, int win = 0, const double* diag_override = nullptr, int rb_mode = 0) {
  check_matrix(A, what);
  D.n_rows = A.n_rows; D.n_cols = A.n_cols; D.br = A.br; D.bc = A.bc;
  D.nnz = A.rowptr[A.n_rows];
  if (rb_mode && (A.br > 1 || A.bc > 1) && try_build_rb(K, A, rb_mode == 2, D)) return;
  const double avg = D.n_rows ? (double)D.nnz / (double)D.n_rows : 0.0;
  D.lanes = pick_lanes(avg);
  // scalar matrices: sliced ELL with G lanes per row; G = the smallest power of two that yields >= 2^20
  // threads (enough waves to fill 256 CUs), accepted if the padding stays below 35 %
  int sellG = 0;
  if (allow_sell && A.br == 1 && A.bc == 1 && D.n_rows > 0 && D.nnz > 0) {
    int G = 1;
    while (G < 16 && D.n_rows * G < ((int64_t)1 << 20) && avg > 3.0 * G) G <<= 1;
    G = std::max(G, sell_long_row_lanes(K, avg));
    if (K.sell_max_lanes) G = std::min(G, K.sell_max_lanes);
    for (int g = G; g >= 1; g >>= 1)
      if ((double)sell_stored(A, g) <= max_pad * (double)D.nnz) { sellG = g; break; }
  }
  // one thread per row with ragged rows: length-sorted windows instead of padding every slice to its longest row.  Short ragged
  // rows whose plain slices pad beyond max_pad (prolongations of the reference's setup: 1 ... 6 entries, 3.3 on average) take the
  // windowed form too if ITS padding is acceptable -- the CSR-vector kernel runs such a P at 2.3 TB/s (263 us at cfg 2)
  // (win < 0: the windowed form only as that fallback, never instead of an acceptable plain SELL image)
  const bool win_fallback_only = win < 0;
  if (win < 0) win = -win;
  bool windowed = win > 0 && !win_fallback_only && sellG == 1 && (double)sell_stored(A, 1) > 1.10 * (double)D.nnz && !K.no_sell_window;
  const bool try_win = win > 0 && sellG == 0 && allow_sell && A.br == 1 && A.bc == 1 && D.n_rows >= 4 * win && D.nnz > 0 && avg <= 12.0 &&
                       !K.no_sell_window && !K.no_sell_window_short;
  std::vector<int32_t> rows;
  std::vector<uint16_t> rowloc;
  if (windowed || try_win) {
    rows.resize((size_t)A.n_rows);
    rowloc.resize((size_t)A.n_rows);
    par_for((A.n_rows + win - 1) / win, [&](int64_t q0, int64_t q1, int) {
      for (int64_t q = q0; q < q1; ++q) {
        const int64_t w0 = q * win, w1 = std::min<int64_t>(A.n_rows, w0 + win);
        for (int64_t i = w0; i < w1; ++i) rows[i] = (int32_t)i;
        std::stable_sort(rows.begin() + w0, rows.begin() + w1, [&](int32_t a, int32_t b) {
          return A.rowptr[a + 1] - A.rowptr[a] > A.rowptr[b + 1] - A.rowptr[b]; });
        for (int64_t i = w0; i < w1; ++i) rowloc[i] = (uint16_t)(rows[i] - w0);
      }
    }, 8);
    if (try_win) {
      int64_t stored = 0;
      for (int64_t sl = 0; sl * WAVE < A.n_rows; ++sl) {           // (sorted windows: the first row of a slice is its longest)
        const int32_t r = rows[sl * WAVE];
        stored += (int64_t)(A.rowptr[r + 1] - A.rowptr[r]) * WAVE;
      }
      windowed = (double)stored <= max_pad * (double)D.nnz;
    }
  }
  if (windowed) {
    HostSell S;
    build_sell(A, rows.data(), A.n_rows, false, 1, S, false);
    D.fmt = FMT_SELL;
    D.lanes = 1;
    D.n_slices = (int)(S.slice_ptr.size() - 1);
    D.stored = S.slice_ptr.back() & ~(int64_t)63;
    D.stream_bytes = S.stream_bytes + 2 * A.n_rows;
    upload_sell(S, D.sell);
    D.sell.win = win;
    D.sell.rowloc.upload(rowloc);
  } else if (sellG) {
    HostSell S;
    build_sell(A, nullptr, A.n_rows, rowrel_ok && A.n_cols >= A.n_rows, sellG, S, rowrel_ok && !K.no_diag_first);
    const bool wdiag = diag_override && S.diag_first && sellG == 1;
    if (wdiag) patch_sell_diag(S, A.n_rows, diag_override);
    D.fmt = FMT_SELL;
    D.lanes = sellG;
    D.n_slices = (int)(S.slice_ptr.size() - 1);
    D.stored = S.slice_ptr.back() & ~(int64_t)63;
    D.stream_bytes = S.stream_bytes;
    upload_sell(S, D.sell);
    D.sell.wdiag = wdiag ? 1 : 0;
  } else {
    D.fmt = FMT_CSRVEC;
    D.stored = D.nnz;
    D.stream_bytes = D.nnz * (8 * (int64_t)A.br * A.bc + 4) + 4 * (A.n_rows + 1);
    // square blocks with near-uniform row lengths: block SELL (one lane per scalar row); the CSR arrays are kept only
    // if a block Gauss-Seidel sweep needs them
    bool bsell = false;
    if (A.br == A.bc && (A.br == 2 || A.br == 3 || A.br == 6) && A.n_rows == A.n_cols && D.nnz > 0 && !K.no_bsell)
      bsell = build_bsell(A, D, 1.30);   // BSELL streams at ~5.6 TB/s vs ~4.0 TB/s of the CSR block kernels: worth up to ~35 % padding
    if (bsell && !keep_csr) return;
    std::vector<int32_t> rp(A.n_rows + 1);
    for (int64_t i = 0; i <= A.n_rows; ++i) rp[i] = (int32_t)A.rowptr[i];
    D.rowptr.upload(rp);
    D.col.upload(A.col, D.nnz);
    D.val.upload(A.val, (size_t)D.nnz * A.br * A.bc);
  }
}

// block Gauss-Seidel data: validated (a wrong block colouring would be a data race), blocks listed colour-major
static void build_bgs(const amgx_level_desc& d, DevLevel& L) {
  const int64_t n = d.A.n_rows;
  const int nb = d.bgs_n_blocks, nc = d.bgs_n_colors;
  if (nb < 0 || (nb > 0 && (!d.bgs_block_ptr || !d.bgs_block_rows || !d.bgs_dinv_ptr || !d.bgs_dinv || !d.bgs_color || nc <= 0)))
    throw Err("AMGX_SM_BGS needs blocks, their inverses and a block colouring (amgx_level_desc.bgs_*)");
  DevBGS& g = L.bgs;
  g.n_colors = nb ? nc : 0;
  std::vector<int32_t> blockof(n, -1);
  const int bs = d.A.br;
  for (int k = 0; k < nb; ++k) {
    const int64_t m = d.bgs_block_ptr[k + 1] - d.bgs_block_ptr[k];
    if (m < 0 || m * bs > BGS_MAX_M) throw Err("block Gauss-Seidel: block with more than 1024 scalar dofs");
    g.max_m = std::max(g.max_m, (int)(m * bs));
    if ((m * bs) * (m * bs) != d.bgs_dinv_ptr[k + 1] - d.bgs_dinv_ptr[k]) throw Err("block Gauss-Seidel: bgs_dinv_ptr does not match the block sizes");
    if (d.bgs_color[k] < 0 || d.bgs_color[k] >= nc) throw Err("block Gauss-Seidel: block colour out of range");
    for (int q = d.bgs_block_ptr[k]; q < d.bgs_block_ptr[k + 1]; ++q) {
      const int32_t i = d.bgs_block_rows[q];
      if (i < 0 || i >= n || blockof[i] >= 0) throw Err("block Gauss-Seidel: blocks must be disjoint sets of valid rows");
      blockof[i] = k;
    }
  }
  for (int64_t i = 0; i < n; ++i) {
    const int k = blockof[i];
    if (k < 0) continue;
    for (int64_t e = d.A.rowptr[i]; e < d.A.rowptr[i + 1]; ++e) {
      const int64_t j = d.A.col[e];
      if (j >= n) continue;            // ghost column: frozen during the sweep
      const int kj = blockof[j];
      if (kj >= 0 && kj != k && d.bgs_color[kj] == d.bgs_color[k]) throw Err("invalid block colouring: two coupled blocks share a colour");
    }
  }
  g.color_ptr.assign(nc + 1, 0);
  for (int k = 0; k < nb; ++k) g.color_ptr[d.bgs_color[k] + 1]++;
  for (int c = 0; c < nc; ++c) g.color_ptr[c + 1] += g.color_ptr[c];
  std::vector<int32_t> list(nb);
  std::vector<int> pos(g.color_ptr.begin(), g.color_ptr.end() - 1);
  for (int k = 0; k < nb; ++k) list[pos[d.bgs_color[k]]++] = k;
  g.blocklist.upload(list);
  g.block_ptr.upload(d.bgs_block_ptr, (size_t)nb + 1);
  g.block_rows.upload(d.bgs_block_rows, (size_t)d.bgs_block_ptr[nb]);
  g.dinv_ptr.upload(d.bgs_dinv_ptr, (size_t)nb + 1);
  g.dinv.upload(d.bgs_dinv, (size_t)d.bgs_dinv_ptr[nb]);
  const int64_t nnz = d.A.rowptr[n];
  if (nnz >= I32_MAX) throw Err("block Gauss-Seidel: too many entries for 32-bit offsets");
  std::vector<int32_t> rp(n + 1);
  for (int64_t i = 0; i <= n; ++i) rp[i] = (int32_t)d.A.rowptr[i];
  g.rowptr.upload(rp);
  g.col.upload(d.A.col, (size_t)nnz);
  g.val.upload(d.A.val, (size_t)nnz * bs * bs);
}

// Compact chunks for the fused pre-smoothing + restriction kernels.  A chunk of 512 CONSECUTIVE rows of a lexicographically numbered
// grid is 2.4 grid lines of one plane, while the fine support of a coarse basis function spans 4 lines x 4 planes: 13 chunks hold a
// piece of every coarse row (cfg 2, reference hierarchy: 16 M partial sums for 1.24 M coarse rows, restrict_sum_kernel 53 us).  The
// matrix image keeps its natural 64-row slices (coalesced streaming, diagonal-first rows, row-relative 16-bit columns); only the
// ASSIGNMENT of slices to workgroups changes: slices that share coarse columns are clustered greedily over the slice graph (shared
// columns of P as weights), spc slices per chunk.  On the grid above a chunk becomes ~64 (x) x 3 x 3: 4-5 partial sums per coarse row.
// Returns the slice list (n_chunks * spc entries, -1 = no slice).  Independent ranges per setup thread (chunks do not cross them).
static std::vector<int32_t> cluster_slices(const amgx_matrix& P, int spc) {
  const int64_t nf = P.n_rows, nc = P.n_cols;
  const int64_t ns = (nf + WAVE - 1) / WAVE;
  // coarse columns of every slice (sorted, unique) and the slices of every coarse column
  std::vector<int64_t> sptr((size_t)ns + 1, 0);
  std::vector<std::vector<int32_t>> scols((size_t)ns);
  par_for(ns, [&](int64_t s0, int64_t s1, int) {
    for (int64_t sl = s0; sl < s1; ++sl) {
      std::vector<int32_t>& u = scols[sl];
      const int64_t r0 = sl * WAVE, r1 = std::min<int64_t>(nf, r0 + WAVE);
      u.assign(P.col + P.rowptr[r0], P.col + P.rowptr[r1]);
      std::sort(u.begin(), u.end());
      u.erase(std::unique(u.begin(), u.end()), u.end());
    }
  }, 64);
  std::vector<int32_t> cptr((size_t)nc + 1, 0);
  for (int64_t sl = 0; sl < ns; ++sl) for (int32_t J : scols[sl]) cptr[J + 1]++;
  for (int64_t J = 0; J < nc; ++J) cptr[J + 1] += cptr[J];
  std::vector<int32_t> cs((size_t)cptr[nc]);
  { std::vector<int32_t> pos(cptr.begin(), cptr.end() - 1); for (int64_t sl = 0; sl < ns; ++sl) for (int32_t J : scols[sl]) cs[pos[J]++] = (int32_t)sl; }
  const int T = std::max(1, std::min<int>(setup_threads(), (int)(ns / (64 * spc) + 1)));
  std::vector<std::vector<int32_t>> lists((size_t)T);
  std::vector<std::thread> th;
  auto work = [&](int t) {
    const int64_t a = ns * t / T, b = ns * (t + 1) / T;
    std::vector<char> done((size_t)(b - a), 0);
    std::vector<int32_t> wgt((size_t)(b - a), 0), touched;
    std::vector<int32_t>& out = lists[t];
    for (int64_t seed = a; seed < b; ++seed) {
      if (done[seed - a]) continue;
      touched.clear();
      int64_t cur = seed;
      for (int q = 0; q < spc; ++q) {
        out.push_back((int32_t)cur);
        done[cur - a] = 1;
        if (q + 1 == spc) break;
        for (int32_t J : scols[cur])
          for (int32_t k = cptr[J]; k < cptr[J + 1]; ++k) {
            const int64_t o = cs[k];
            if (o < a || o >= b || done[o - a]) continue;
            if (wgt[o - a]++ == 0) touched.push_back((int32_t)o);
          }
        int64_t best = -1;
        int32_t bw = 0;
        for (int32_t o : touched) if (!done[o - a] && (wgt[o - a] > bw || (wgt[o - a] == bw && bw > 0 && o < best))) { bw = wgt[o - a]; best = o; }
        if (best < 0) {                                        // nothing adjacent is left: take the next free slice in order
          for (int64_t o = seed + 1; o < b; ++o) if (!done[o - a]) { best = o; break; }
          if (best < 0) { for (int r = q + 1; r < spc; ++r) out.push_back(-1); break; }
        }
        cur = best;
      }
      for (int32_t o : touched) wgt[o - a] = 0;
    }
  };
  for (int t = 1; t < T; ++t) th.emplace_back(work, t);
  work(0);
  for (auto& x : th) x.join();
  std::vector<int32_t> list;
  for (int t = 0; t < T; ++t) list.insert(list.end(), lists[t].begin(), lists[t].end());
  return list;
}

// CH = fine rows per chunk; threads = workgroup size of the kernel that consumes the chunk (= CH unless several lanes share a row)
// slice_list (optional, one thread per row only): chunk c = the 64-row slices slice_list[c * CH / 64 ...) (cluster_slices)
// runs (optional, instead of a slice list): chunk c = the rows of the runs runs->run_ptr[c] .. runs->run_ptr[c + 1) (box chunks of
// the diagonal image); the local index counts through the runs in their order, CH = the rows of the fullest chunk
static void build_restrict(const Knobs& K, const amgx_matrix& P, DevRestrict& R, int CH = RESTRICT_CHUNK, int max_entries = RESTRICT_MAX_ENTRIES, int threads = 0,
                           const std::vector<int32_t>* slice_list = nullptr, const dia::BoxRuns* runs = nullptr) {
  if (threads <= 0) threads = CH;
  const int64_t nf = P.n_rows, nc = P.n_cols;
  const int spc = CH / WAVE;
  if (slice_list && (runs || CH % WAVE != 0 || slice_list->size() % spc != 0)) throw Err("build_restrict: slice list does not match the chunk size");
  if (runs) {
    int64_t covered = 0;
    for (int64_t c = 0; c < runs->n_boxes(); ++c) {
      int64_t rows = 0;
      for (int64_t q = runs->run_ptr[c]; q < runs->run_ptr[c + 1]; ++q) {
        if (runs->first[q] < 0 || runs->len[q] < 0 || runs->first[q] + runs->len[q] > nf) throw Err("build_restrict: a run leaves the level");
        rows += runs->len[q];
      }
      if (rows > CH || rows > 65536) throw Err("build_restrict: a chunk of runs has more rows than its local index holds");
      covered += rows;
    }
    if (covered != nf) throw Err("build_restrict: the runs do not cover the level's rows once");
  }
  const int64_t nch = runs ? runs->n_boxes() : slice_list ? (int64_t)slice_list->size() / spc : (nf + CH - 1) / CH;
  // pass 1 (parallel over chunks): slots (= distinct coarse columns) per chunk; a chunk's entries are the P entries of its rows
  std::vector<int32_t> chunk_slot(nch + 1, 0);
  std::vector<char> too_long(setup_threads(), 0);
  std::vector<int64_t> fullest(setup_threads(), 0);
  struct Trip { int32_t J; uint16_t i; double w; };
  auto chunk_trips = [&](int64_t c, std::vector<Trip>& t) {
    t.clear();
    if (runs) {
      int64_t local = 0;
      for (int64_t q = runs->run_ptr[c]; q < runs->run_ptr[c + 1]; ++q)
        for (int64_t i = runs->first[q]; i < runs->first[q] + runs->len[q]; ++i, ++local) {
          for (int64_t k = P.rowptr[i]; k < P.rowptr[i + 1]; ++k) t.push_back({P.col[k], (uint16_t)local, P.val[k]});
        }
    } else if (slice_list) {
      for (int q = 0; q < spc; ++q) {
        const int64_t sl = (*slice_list)[c * spc + q];
        if (sl < 0) continue;
        const int64_t r0 = sl * WAVE, r1 = std::min<int64_t>(nf, r0 + WAVE);
        for (int64_t i = r0; i < r1; ++i)
          for (int64_t k = P.rowptr[i]; k < P.rowptr[i + 1]; ++k) t.push_back({P.col[k], (uint16_t)(q * WAVE + (i - r0)), P.val[k]});
      }
    } else {
      const int64_t r0 = c * CH, r1 = std::min<int64_t>(nf, r0 + CH);
      for (int64_t i = r0; i < r1; ++i)
        for (int64_t k = P.rowptr[i]; k < P.rowptr[i + 1]; ++k) t.push_back({P.col[k], (uint16_t)(i - r0), P.val[k]});
    }
    std::stable_sort(t.begin(), t.end(), [](const Trip& a, const Trip& b) { return a.J < b.J; });
  };
  std::vector<int64_t> chunk_ent(nch + 1, 0);            // first entry of every chunk
  par_for(nch, [&](int64_t c0, int64_t c1, int tid) {
    std::vector<Trip> t;
    for (int64_t c = c0; c < c1; ++c) {
      chunk_trips(c, t);
      if ((int64_t)t.size() > max_entries) { too_long[tid] = 1; return; }
      fullest[tid] = std::max<int64_t>(fullest[tid], (int64_t)t.size());
      int32_t nsl = 0;
      for (size_t q = 0; q < t.size(); ++q) if (q == 0 || t[q].J != t[q - 1].J) nsl++;
      chunk_slot[c + 1] = nsl;
      chunk_ent[c + 1] = (int64_t)t.size();
    }
  }, 8);
  for (char c : too_long) if (c) return;             // rows too long for the LDS product buffer: keep the P^T form
  for (int64_t c = 0; c < nch; ++c) { chunk_slot[c + 1] += chunk_slot[c]; chunk_ent[c + 1] += chunk_ent[c]; }
  const int64_t n_slots = chunk_slot[nch], n_ent = P.rowptr[nf];
  std::vector<int32_t> slot_ptr((size_t)n_slots + 1, 0), slot_col((size_t)n_slots);
  std::vector<double> w((size_t)n_ent);
  std::vector<uint16_t> fi((size_t)n_ent);
  // pass 2: fill (entries of chunk c start at chunk_ent[c])
  par_for(nch, [&](int64_t c0, int64_t c1, int) {
    std::vector<Trip> t;
    for (int64_t c = c0; c < c1; ++c) {
      chunk_trips(c, t);
      int64_t e = chunk_ent[c];
      int64_t sl = chunk_slot[c];
      for (size_t q = 0; q < t.size(); ++q) {
        if (q == 0 || t[q].J != t[q - 1].J) { slot_ptr[sl] = (int32_t)e; slot_col[sl] = t[q].J; sl++; }
        w[e] = t[q].w; fi[e] = t[q].i; e++;
      }
    }
  }, 8);
  slot_ptr[n_slots] = (int32_t)n_ent;
  const int64_t ns = (int64_t)slot_col.size();
  if ((int64_t)slot_ptr.size() != ns + 1) throw Err("build_restrict: internal slot count mismatch");
  std::vector<int32_t> optr(nc + 1, 0), oidx(ns);
  for (int64_t sidx = 0; sidx < ns; ++sidx) optr[slot_col[sidx] + 1]++;
  for (int64_t J = 0; J < nc; ++J) optr[J + 1] += optr[J];
  std::vector<int32_t> pos(optr.begin(), optr.end() - 1);
  for (int64_t sidx = 0; sidx < ns; ++sidx) oidx[pos[slot_col[sidx]]++] = (int32_t)sidx;   // ascending chunk order per row
  R.n_chunks = (int)nch; R.n_slots = ns;
  int64_t mx_chunk = 0;
  for (int64_t v : fullest) mx_chunk = std::max(mx_chunk, v);
  for (int64_t c = 0; c < nch; ++c) R.max_slots = std::max(R.max_slots, chunk_slot[c + 1] - chunk_slot[c]);
  R.max_entries = mx_chunk;
  // entries of P per thread: the smallest value of the kernels' list (down_plan.hpp) that holds the fullest chunk.  This is the
  // guard against a kernel that would drop entries: a caller whose max_entries admits more than the list's last value holds
  // fails here (make_down_plan then only asks whether the value belongs to the list of the kernel that was chosen)
  auto ept_of = [&](auto list) {
    for (int e : values(list)) if (mx_chunk <= (int64_t)e * threads) return e;
    throw Err("build_restrict: no listed EPT holds the fullest chunk");
  };
  // local-window chunks (lw_image, build_gsb_images): DOWN_THREADS lanes, a listed number of them per row, the list's last EPT
  const bool lw = threads == DOWN_THREADS && threads % CH == 0 && contains(DownLwLanes{}, threads / CH) &&
                  max_entries == values(DownLwEpt{}).back() * DOWN_THREADS;
  if (runs) R.ept = (int)std::max<int64_t>(1, (mx_chunk + threads - 1) / threads);     // (the box kernel loops: any number of entries per lane)
  else R.ept = lw ? ept_of(DownLwEpt{}) : ept_of(DownEpt{});
  if (R.ept > K.fused_ept_max) { R = DevRestrict(); return; }     // (A/B hook: keep the separate kernels instead)
  R.chunk_slot.upload(chunk_slot); R.slot_ptr.upload(slot_ptr); R.optr.upload(optr);
  // Measured NON-win (profiles/r01/restrict_fused.txt): storing the partial sums row by row (scattered stores in the
  // producer, streaming loads in restrict_sum_kernel) makes the cycle 2-4 % slower at cfg 2; off unless AMGX_RSUM_SORT=1.
  if (!K.rsum_sort) R.oidx.upload(oidx);
  else {
    std::vector<int32_t> dest(ns);
    for (int64_t k = 0; k < ns; ++k) dest[oidx[k]] = (int32_t)k;
    R.dest.upload(dest);
  }
  R.w.upload(w); R.fi.upload(fi);
  R.part.alloc((size_t)std::max<int64_t>(1, ns));
  if (slice_list) R.slice_list.upload(*slice_list);
}

// the chunk-local P^T of a fused down kernel: chunks of rows_per_chunk rows with up to `entries` entries of P, `threads` lanes per
// workgroup.  The one place that decides between compact chunks (cluster_slices) and consecutive ones: compact where the caller's
// own precondition (`compact`) holds and the level has AMGX_COMPACT_CHUNKS_MIN_ROWS rows
static void build_restrict_chunks(const Knobs& K, const amgx_matrix& P, DevRestrict& R, int rows_per_chunk, int entries, int threads, bool compact) {
  if (compact && K.compact_chunks_wanted(P.n_rows)) {
    const std::vector<int32_t> sl = cluster_slices(P, rows_per_chunk / WAVE);
    build_restrict(K, P, R, rows_per_chunk, entries, threads, &sl);
  } else
    build_restrict(K, P, R, rows_per_chunk, entries, threads);
}

// "local window" image of a long-row scalar matrix (sell_lw_pre_restrict_kernel): per chunk of LW_ROWS consecutive rows the sorted
// list of its distinct columns; the SELL-2 image stores indices into that list.  vals: the (scaled) values in CSR order.
// Returns false (nothing built) if a chunk touches more than LW_CAP distinct columns.
static bool build_sell_lw(const Knobs& K, const amgx_matrix& A, const double* vals, int G, DevMatrix& D, DevBuf<int32_t>& d_cptr, DevBuf<int32_t>& d_ccol) {
  const int64_t n = A.n_rows, nnz = A.rowptr[n];
  const int LW_ROWS = 512 / G;
  const int64_t nch = (n + LW_ROWS - 1) / LW_ROWS;
  std::vector<int32_t> cnt((size_t)nch + 1, 0);
  RawVec<int32_t> lcol;
  lcol.resize((size_t)std::max<int64_t>(1, nnz));
  std::vector<std::vector<int32_t>> lists((size_t)nch);
  std::vector<char> no16((size_t)n, 0);                 // rows of chunks whose window would not fit: global 32-bit columns, no window
  const int64_t cap = K.lw_cap(LW_CAP);
  const bool tcap = K.lw_test_cap_on;
  std::vector<int64_t> n_over(setup_threads(), 0);
  par_for(nch, [&](int64_t c0, int64_t c1, int t) {
    std::vector<int32_t> u;
    for (int64_t c = c0; c < c1; ++c) {
      const int64_t r0 = c * LW_ROWS, r1 = std::min<int64_t>(n, r0 + LW_ROWS);
      u.assign(A.col + A.rowptr[r0], A.col + A.rowptr[r1]);
      std::sort(u.begin(), u.end());
      u.erase(std::unique(u.begin(), u.end()), u.end());
      if ((int64_t)u.size() > cap) {
        for (int64_t i = r0; i < r1; ++i) no16[i] = 1;
        for (int64_t k = A.rowptr[r0]; k < A.rowptr[r1]; ++k) lcol[k] = A.col[k];
        n_over[t]++;
        continue;
      }
      for (int64_t k = A.rowptr[r0]; k < A.rowptr[r1]; ++k) lcol[k] = (int32_t)(std::lower_bound(u.begin(), u.end(), A.col[k]) - u.begin());
      cnt[c + 1] = (int32_t)u.size();
      lists[c] = u;
    }
  }, 4);
  int64_t overs = 0;
  for (int64_t v : n_over) overs += v;
  if (overs * 20 > nch && !tcap) return false;          // (more than 5 % of the chunks without a window: the plain image is the better choice)
  for (int64_t c = 0; c < nch; ++c) cnt[c + 1] += cnt[c];
  std::vector<int32_t> ccol((size_t)std::max<int32_t>(1, cnt[nch]));
  par_for(nch, [&](int64_t c0, int64_t c1, int) { for (int64_t c = c0; c < c1; ++c) std::copy(lists[c].begin(), lists[c].end(), ccol.begin() + cnt[c]); }, 64);
  amgx_matrix L = A;
  L.col = lcol.data();
  L.val = vals;
  HostSell S;
  build_sell(L, nullptr, n, false, G, S, false, &no16);
  const int64_t ns = (int64_t)S.slice_ptr.size() - 1;
  // (every slice of a chunk with a window fits 16-bit deltas by construction: indices < LW_CAP; anything else would be a builder bug)
  int64_t want16 = 0;
  for (int64_t sl = 0; sl < ns; ++sl) if (!no16[std::min<int64_t>(n - 1, sl * (WAVE / G))]) ++want16;
  if (S.n_comp_slices != want16) return false;
  D.n_rows = n; D.n_cols = A.n_cols; D.br = D.bc = 1; D.nnz = nnz;
  D.fmt = FMT_SELL; D.lanes = G;
  D.n_slices = (int)ns;
  D.stored = S.slice_ptr.back() & ~(int64_t)63;
  D.stream_bytes = S.stream_bytes + 4 * (int64_t)ccol.size() + 4 * (nch + 1);
  upload_sell(S, D.sell);
  d_cptr.upload(cnt);
  d_ccol.upload(ccol);
  return true;
}

// local-window form of a WINDOWED SELL image (sell_lw_win_spmv_kernel): windows of SELL_WIN consecutive rows stored by decreasing
// length as in upload_matrix, columns = indices into the window's sorted list of distinct columns (at most QW_CAP; windows beyond
// that keep 32-bit global columns).  rowptr / col / val: host CSR.  Returns false if too many windows miss the capacity.
static bool build_sell_lw_windowed(const Knobs& K, int64_t n, int64_t n_cols, const int64_t* rowptr, const int32_t* col, const double* val, DevMatrix& D,
                                   DevBuf<int32_t>& d_cptr, DevBuf<int32_t>& d_ccol) {
  const int win = SELL_WIN;
  const int64_t nnz = rowptr[n];
  const int64_t nw = (n + win - 1) / win;
  SetupClock clk(K);
  std::vector<int32_t> cnt((size_t)nw + 1, 0);
  RawVec<int32_t> lcol;
  lcol.resize((size_t)std::max<int64_t>(1, nnz));
  std::vector<std::vector<int32_t>> lists((size_t)nw);
  std::vector<char> no16((size_t)n, 0);
  std::vector<int32_t> rows((size_t)n);
  std::vector<uint16_t> rowloc((size_t)n);
  std::vector<int64_t> n_over(setup_threads(), 0);
  const int64_t cap = K.lw_cap_small(QW_CAP);
  const bool tcap = K.lw_test_cap_on;
  par_for(nw, [&](int64_t q0, int64_t q1, int t) {
    std::vector<int32_t> u;
    for (int64_t q = q0; q < q1; ++q) {
      const int64_t w0 = q * win, w1 = std::min<int64_t>(n, w0 + win);
      for (int64_t i = w0; i < w1; ++i) rows[i] = (int32_t)i;
      std::stable_sort(rows.begin() + w0, rows.begin() + w1, [&](int32_t a, int32_t b) { return rowptr[a + 1] - rowptr[a] > rowptr[b + 1] - rowptr[b]; });
      for (int64_t i = w0; i < w1; ++i) rowloc[i] = (uint16_t)(rows[i] - w0);
      u.assign(col + rowptr[w0], col + rowptr[w1]);
      std::sort(u.begin(), u.end());
      u.erase(std::unique(u.begin(), u.end()), u.end());
      if ((int64_t)u.size() > cap) {
        for (int64_t i = w0; i < w1; ++i) no16[i] = 1;
        for (int64_t k = rowptr[w0]; k < rowptr[w1]; ++k) lcol[k] = col[k];
        n_over[t]++;
        continue;
      }
      for (int64_t k = rowptr[w0]; k < rowptr[w1]; ++k) lcol[k] = (int32_t)(std::lower_bound(u.begin(), u.end(), col[k]) - u.begin());
      cnt[q + 1] = (int32_t)u.size();
      lists[q] = u;
    }
  }, 4);
  clk.lap("  lw-win: window lists + local columns");
  int64_t overs = 0;
  for (int64_t v : n_over) overs += v;
  if (overs * 20 > nw && !tcap) return false;
  for (int64_t q = 0; q < nw; ++q) cnt[q + 1] += cnt[q];
  std::vector<int32_t> ccol((size_t)std::max<int32_t>(1, cnt[nw]));
  par_for(nw, [&](int64_t q0, int64_t q1, int) { for (int64_t q = q0; q < q1; ++q) std::copy(lists[q].begin(), lists[q].end(), ccol.begin() + cnt[q]); }, 64);
  amgx_matrix L{};
  L.n_rows = n; L.n_cols = n_cols; L.br = L.bc = 1;
  L.rowptr = rowptr; L.col = lcol.data(); L.val = val;
  clk.lap("  lw-win: list copy");
  HostSell S;
  build_sell(L, rows.data(), n, false, 1, S, false, &no16);
  clk.lap("  lw-win: host SELL builder");
  D.n_rows = n; D.n_cols = n_cols; D.br = D.bc = 1; D.nnz = nnz;
  D.fmt = FMT_SELL; D.lanes = 1;
  D.n_slices = (int)(S.slice_ptr.size() - 1);
  D.stored = S.slice_ptr.back() & ~(int64_t)63;
  D.stream_bytes = S.stream_bytes + 2 * n + 4 * (int64_t)ccol.size() + 4 * (nw + 1);
  upload_sell(S, D.sell);
  D.sell.win = win;
  D.sell.rowloc.upload(rowloc);
  d_cptr.upload(cnt);
  d_ccol.upload(ccol);
  clk.lap("  lw-win: upload");
  return true;
}

// ---------------------------------------------------------------------------------------------------
// the handle
// ---------------------------------------------------------------------------------------------------

struct MultiState;                      // multi-vector work space and captured graphs (multi.hpp)
void multi_drop_graphs(MultiState* s);
void multi_free(MultiState* s);
struct MvState;                         // work space of the multi-vector algebra calls (mv.hpp)
void mv_free(MvState* s);

struct Handle {
  int device = 0;
  Knobs knobs;                          // the switches as amgx_create found them (knobs.hpp)
  std::vector<DevLevel> lev;
  int cycle = AMGX_CYCLE_V, clev = AMGX_CLEV_INV;
  int64_t coarse_n = 0;
  int64_t coarse_ld = 0;                // row stride of coarse_inv (== coarse_n for an inverse handed over by the host)
  double coarse_pivot = 0.0;            // device-side inversion: smallest pivot ratio met (dense_spd.hpp)
  DevBuf<double> coarse_inv;
  hipStream_t own_stream = nullptr, stream = nullptr;
  bool use_graph = true;
  bool skip_rsum = false;               // amgx_time_op(op 7): time sell_pre_restrict_kernel alone
  // amgx_time_op(op 8): HIP events around the fused down kernel of `probe_level` INSIDE the cycle (direct launches)
  // (op 9): the same around the backward block-hybrid Gauss-Seidel sweep of `probe_level`
  int probe_level = -1, probe_kind = 8;
  hipEvent_t probe_e0 = nullptr, probe_e1 = nullptr;
  int ep_nt = 1;                        // non-temporal epilogue operands (AMGX_NO_EP_NT=1 disables)
  int tail_level = -1;                  // first level executed by tail_kernel (-1: no fused tail)
  int tail_ops = 0;
  std::vector<int> tail_gs_lds;         // per level: form of its Gauss-Seidel sweeps inside tail_kernel (1: x in LDS, 0: x in global memory,
                                        //   -1: the level has no such sweep); amgx_level_extra reports it
  DevBuf<TailOp> tail_prog;
  // collapsed coarse levels (kernels.hpp, dense_op_gemv_kernel): the V-cycle on the levels >= dense_level as ONE dense
  // operator, formed at create time by the device's own sub-cycle on the unit vectors (build_dense_tail)
  int dense_level = -1;
  int dense_n = 0, dense_ld = 0;
  DevBuf<double> dense_op;
  std::string err;
  struct GraphKey { const double* b; double* x; int kind; bool operator<(const GraphKey& o) const { return std::tie(b, x, kind) < std::tie(o.b, o.x, o.kind); } };
  GraphCache<GraphKey> graphs;
  MultiState* multi = nullptr;          // created by the first multi-vector call (multi.hpp)
  MvState* mv = nullptr;                // created by the first amgx_mv_gram / amgx_mv_combine (mv.hpp)
  // staging for host-pointer calls
  DevBuf<double> stage[3];
  DevBuf<double> kr_ws[6];              // work vectors of amgx_pcg / amgx_gmres (krylov.hpp), kept between solves
  DevBuf<double> stage_raw[3];          // host vectors of permuted levels: raw copy before / after the renumbering
  // Gauss-Seidel levels are stored in colour-major numbering (see LevelPerm in create()); perm[l][new] = old row of the
  // caller's numbering, empty = identity.  Every C-ABI entry point translates its vectors (struct Staged).
  std::vector<DevBuf<int32_t>> perm;
  bool permuted(int l) const { return l >= 0 && l < (int)perm.size() && perm[l].n > 0; }
  void perm_gather(int l, const double* src, double* dst) {
    const int64_t len = lev[l].len();
    if (!len) return;
    launch(perm_gather_kernel, grid_for(len), BLOCK, 0, stream, len, lev[l].bs, perm[l].p, src, dst);
  }
  void perm_scatter(int l, const double* src, double* dst) {
    const int64_t len = lev[l].len();
    if (!len) return;
    launch(perm_scatter_kernel, grid_for(len), BLOCK, 0, stream, len, lev[l].bs, perm[l].p, src, dst);
  }

  ~Handle() {
    if (multi) multi_free(multi);
    if (mv) mv_free(mv);
    graphs.drop();
    if (own_stream) (void)hipStreamDestroy(own_stream);
  }

  int n_levels() const { return (int)lev.size(); }

  // ------------------------------------------------------------------ primitive ops (all async on `stream`)
  static int grid_for(int64_t threads) { return (int)std::max<int64_t>(1, (threads + BLOCK - 1) / BLOCK); }
  // workgroups of the kernels that give every unit (a slice, a row of a dense matrix) one wave
  static int wave_grid(int64_t units) { return (int)((units + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK); }

  // Part of the rows a launch covers: Span and unit_range (down_plan.hpp).  Formats that cannot be split run completely in the
  // boundary part (correct, no overlap).
  using Span = ::amgx::Span;
  enum { PART_ALL = ::amgx::PART_ALL, PART_INT = ::amgx::PART_INT, PART_BND = ::amgx::PART_BND };

  // ------------------------------------------------------------------ the product launcher
  // The value lists of the product kernels, each written once: product() dispatches on them and the multi-vector path asks them
  // whether a kernel exists (multi_*_ok), so a shape cannot be in one place and not in the other.  Shapes: key = 10 * br + bc.
  using SquareShapes = IntList<22, 33, 66>;                                             // EP_JAC / EP_CHEB: square blocks only
  using RowlaneShapes = IntList<22, 33, 66, 36, 63, 23, 32>;                            // bcsr_rowlane_kernel, bcsr_spmm_kernel
  using BcsrVecShapes = IntList<22, 33, 66, 36, 63, 23, 32, 13, 31, 16, 61, 12, 21>;    // bcsrvec_spmv_kernel
  using BsellSizes = IntList<6, 3, 2>;
  using SellLanes = IntList<1, 2, 4, 8>;          // any other lane count: the 16-lane kernel
  using CsrLanes = IntList<2, 4, 8, 16, 32>;      // any other lane count: one wave per row

  // what product<NV > 1> serves: scalar SELL / CSR-vector; block CSR (`square`: under EP_JAC / EP_CHEB); level matrices; transfers
  static bool multi_scalar_ok(const DevMatrix& M) { return M.br == 1 && M.bc == 1 && (M.fmt == FMT_SELL || M.fmt == FMT_CSRVEC); }
  static bool multi_bcsr_ok(const DevMatrix& M, bool square) {
    const int key = M.br * 10 + M.bc;
    return M.fmt == FMT_CSRVEC && (square ? contains(SquareShapes{}, key) : contains(RowlaneShapes{}, key));
  }
  static bool multi_level_ok(const DevMatrix& M) {
    if (M.br != M.bc) return false;
    if (M.br == 1) return multi_scalar_ok(M);
    return M.fmt == FMT_BSELL ? contains(BsellSizes{}, M.br) : multi_bcsr_ok(M, true);
  }
  static bool multi_transfer_ok(const DevMatrix& M) { return M.fmt == FMT_RB || (M.br == 1 && M.bc == 1 ? multi_scalar_ok(M) : multi_bcsr_ok(M, false)); }

  // rigid-body transfer blocks: (fine block, coarse block, dimension of Q) = 663, 363, 332, 232, else 220
  template <class F>
  static void rb_shape(const DevMatrix::Rb& R, F&& run) {
    if (R.dim == 3 && R.bf == 6) run(Int<6>{}, Int<6>{}, Int<3>{});
    else if (R.dim == 3) run(Int<3>{}, Int<6>{}, Int<3>{});
    else if (R.dim == 2 && R.bf == 3) run(Int<3>{}, Int<3>{}, Int<2>{});
    else if (R.dim == 2) run(Int<2>{}, Int<3>{}, Int<2>{});
    else run(Int<2>{}, Int<2>{}, Int<0>{});
  }
  // workgroups of the kernels that give every block row of br scalar rows W lane groups
  static int rowlane_grid(int64_t n_rows, int br, int W) {
    const int rpw = WAVE / (br * W);
    return std::max(1, wave_grid((n_rows + rpw - 1) / rpw));
  }

  // y = EP(M x) on NV vectors: NV == 1 the single-vector kernels (kernels.hpp), NV == 2, 4 their forms on interleaved vectors
  // (multi_kernels.hpp).  One branch per format; in it the unit of the row split, the grid and the value list are written once.
  // sm_pass: a product the smoother or the cycle launches on a level (EP_CHEB steps, the residual after smoothing).  It reads the
  // single-precision image where amgx_create gave the level one (DevMatrix::has32); every other caller reads the fp64 image.
  template <int NV, int EP>
  void product(const DevMatrix& M, const double* x, double* y, const EpArgs& ep, const Span sp = Span(), bool sm_pass = false) {
    static_assert(NV == 1 || EP != EP_PRE, "EP_PRE is built for single vectors only");
    if (M.n_rows == 0) return;
    if (NV > 1 && sp.part != PART_ALL) throw Err("multi-vector product: rank-partitioned levels are not supported");
    // the float image exists for non-windowed SELL and BSELL, under EP_RES / EP_CHEB; for BSELL also under EP_MULT on one vector
    // (r = rest x of a Gauss-Seidel block level)
    // for SELL, on one vector, also under the epilogues of a scalar Jacobi level's passes (EP_PRE on A', EP_JAC on A, EP_AXPY on Q; 5.20)
    constexpr bool EP32 = EP == EP_RES || EP == EP_CHEB;
    // ... and under EP_CRES on `rest` of a scalar Gauss-Seidel level (plain and windowed sliced-ELL; 5.21).  EP_CRES and the EP_MULT of
    // BSELL are built on NV > 1 too: the residual after the fused sweep from zero on float images (5.22)
    constexpr bool EP32_SELL = EP32 || EP == EP_CRES || (NV == 1 && (EP == EP_PRE || EP == EP_JAC || EP == EP_AXPY));
    constexpr bool EP32_WIN = EP == EP_CRES;
    constexpr bool EP32_BSELL = EP32 || EP == EP_MULT;
    const bool f32 = sm_pass && M.has32() && (EP32 || (EP32_SELL && M.fmt == FMT_SELL) || (EP32_BSELL && M.fmt == FMT_BSELL));
    if (f32 && !((M.fmt == FMT_SELL && (!M.sell.win || EP32_WIN)) || M.fmt == FMT_BSELL)) throw Err("single-precision image on a format that has none");
    // run(view of the image this product reads); has32: a float kernel is instantiated for this format and epilogue
    auto image = [&](auto has32, const auto& v64, const auto& v32, auto&& run) {
      if constexpr (decltype(has32)::value) { if (f32) { run(v32); return; } }
      // (a scalar Jacobi level with single-precision images keeps only the float values of A', Q: DESIGN.md 5.20)
      if (!v64.val && M.has32()) throw Err("product: the fp64 values of this image were released (single-precision Jacobi or Gauss-Seidel images); only the passes of the level read it");
      run(v64);
    };
    int64_t a, b;                                     // the units [a, b) of the row split that this launch covers
    if (M.fmt == FMT_RB) {
      if constexpr (EP != EP_MULT && EP != EP_AXPY) throw Err("rigid-body transfer blocks: y = M x and y = yin + s M x only");
      else {
        if (sp.part == PART_INT) return;             // (not split: everything runs in the boundary part)
        const DevMatrix::Rb& R = M.rb;
        const RbMat V = R.view();
        rb_shape(R, [&](auto BF, auto BC, auto DM) {
          constexpr int G = 16;                       // lanes per coarse row of the transposed form
          if constexpr (NV == 1) {
            if (!R.transposed) launch(rb_prolong_kernel<BF(), BC(), DM(), EP>, grid_for(M.n_rows), BLOCK, 0, stream, M.n_rows, V, x, y, ep);
            else launch(rb_restrict_kernel<BF(), BC(), DM(), G, EP>, grid_for(M.n_rows * G), BLOCK, 0, stream, M.n_rows, V, x, y, ep);
          } else {
            if (!R.transposed) launch(rb_prolong_nv_kernel<BF(), BC(), DM(), NV, EP>, grid_for(M.n_rows), BLOCK, 0, stream, M.n_rows, V, x, y, ep);
            else launch(rb_restrict_nv_kernel<BF(), BC(), DM(), G, NV, EP>, grid_for(M.n_rows * G), BLOCK, 0, stream, M.n_rows, V, x, y, ep);
          }
        });
      }
    } else if (M.fmt == FMT_SELL && M.sell.win) {
      if (M.sell.win != SELL_WIN) throw Err("windowed SELL: unexpected window size");
      unit_range(sp, SELL_WIN, (M.n_rows + SELL_WIN - 1) / SELL_WIN, a, b);
      if (b <= a) return;
      // (a smoother pass reads the rounded values of A at fp64 width where the level has them, see val64r)
      image(std::bool_constant<EP32_WIN>{}, sm_pass && M.val64r.p ? M.sell.view_of(M.val64r.p) : M.sell.view(), M.sell.view32(M.val32.p), [&](auto V) {
        using T = std::remove_const_t<std::remove_pointer_t<decltype(V.val)>>;       // double / float
        if constexpr (NV == 1) launch(sell_win_spmv_kernel<SELL_WIN, EP, T>, (int)(b - a), SELL_WIN, 0, stream, M.n_rows, (int)a, V, M.sell.rowloc.p, x, y, ep);
        else launch(sell_win_spmm_kernel<SELL_WIN, NV, EP, T>, (int)(b - a), SELL_WIN, 0, stream, M.n_rows, V, M.sell.rowloc.p, x, y, ep);
      });
    } else if (M.fmt == FMT_SELL) {
      unit_range(sp, WAVE / M.lanes, M.n_slices, a, b);
      if (b <= a) return;
      const int grid = wave_grid(b - a);
      // (AMGX_JACOBI_PREC_F32_WIDE: a Jacobi pass reads the rounded values of A at fp64 width)
      image(std::bool_constant<EP32_SELL>{}, sm_pass && M.val64r.p ? M.sell.view_of(M.val64r.p) : M.sell.view(), M.sell.view32(M.val32.p), [&](auto V) {
        using T = std::remove_const_t<std::remove_pointer_t<decltype(V.val)>>;       // double / float
        auto run = [&](auto G) {
          if constexpr (NV == 1) launch(sell_spmv_kernel<G(), EP, T>, grid, BLOCK, 0, stream, M.n_rows, (int)a, (int)b, V, x, y, ep);
          else launch(sell_spmm_kernel<G(), NV, EP, T>, grid, BLOCK, 0, stream, M.n_rows, M.n_slices, V, x, y, ep);
        };
        if (!dispatch(SellLanes{}, M.lanes, run)) run(Int<16>{});
      });
    } else if (M.br == 1 && M.bc == 1) {
      unit_range(sp, 1, M.n_rows, a, b);
      if (b <= a) return;
      const int grid = grid_for((b - a) * M.lanes);
      const double* const sval = sm_pass && M.val64r.p ? M.val64r.p : M.val.p;       // (a smoother pass: the rounded values, see val64r)
      auto run = [&](auto G) {
        if constexpr (NV == 1) launch(csrvec_spmv_kernel<G(), EP>, grid, BLOCK, 0, stream, a, b, M.rowptr.p, M.col.p, sval, x, y, ep);
        else launch(csrvec_spmm_kernel<G(), NV, EP>, grid, BLOCK, 0, stream, M.n_rows, M.rowptr.p, M.col.p, sval, x, y, ep);
      };
      if (!dispatch(CsrLanes{}, M.lanes, run)) run(Int<64>{});
    } else if constexpr (EP == EP_PRE) {
      throw Err("EP_PRE is only built for scalar matrices");
    } else if constexpr (NV > 1 && EP == EP_CRES) {
      throw Err("multi-vector product: EP_CRES is only built for scalar matrices");
    } else if (M.fmt == FMT_BSELL) {
      // units of RB = 64 / bs block rows (one slice); slices that straddle n_int belong to the boundary part
      unit_range(sp, WAVE / M.br, M.n_slices, a, b);
      if (b <= a) return;
      const int grid = wave_grid(b - a);
      const int xmode = NV == 1 ? knobs.bsell_xmode : 0;       // (the gather variants rearrange loads that the NV > 1 kernel does not have)
      // (AMGX_GS_F32_WIDE: a smoother pass reads the rounded values at fp64 width)
      image(std::bool_constant<EP32_BSELL>{}, M.bsell.view_of(sm_pass && M.val64r.p ? M.val64r.p : M.bsell.val.p, xmode), M.bsell.view32(M.val32.p, xmode), [&](auto V) {
        using T = std::remove_const_t<std::remove_pointer_t<decltype(V.val)>>;
        auto run = [&](auto BS) {
          if constexpr (NV == 1) launch(bsell_spmv_kernel<BS(), EP, T>, grid, BLOCK, 0, stream, M.n_rows, (int)a, (int)b, V, x, y, ep);
          else launch(bsell_spmm_kernel<BS(), NV, EP, T>, grid, BLOCK, 0, stream, M.n_rows, M.n_slices, V, x, y, ep);
        };
        if (dispatch(BsellSizes{}, M.br, run)) return;
        if (NV > 1 || f32) throw Err("unsupported BSELL block size " + std::to_string(M.br));
        run(Int<2>{});                                // single vector, fp64 image: any other block size takes the 2 x 2 kernel
      });
    } else if (sp.part == PART_INT) {
      return;                                         // the CSR block formats are not split: everything runs in the boundary part
    } else {
      // NV == 1: bcsr_kernel() chooses between the row-lane and the vector form; NV > 1: ONE kernel, W = 4 lane groups per block row
      constexpr bool SQ = EP == EP_JAC || EP == EP_CHEB;
      const BcsrKernel bk = NV == 1 ? bcsr_kernel(M, SQ) : BcsrKernel{true, 4};
      const double* const mval = sm_pass && M.val64r.p ? M.val64r.p : M.val.p;       // (a smoother pass: the rounded values, see val64r)
      const int key = M.br * 10 + M.bc;
      bool ok = true;
      if (bk.rowlane) {
        auto run = [&](auto KEY) {
          constexpr int BR = KEY() / 10, BC = KEY() % 10;
          if constexpr (NV == 1) {
            auto run_w = [&](auto W) { launch(bcsr_rowlane_kernel<BR, BC, W(), EP>, rowlane_grid(M.n_rows, BR, W()), BLOCK, 0, stream, M.n_rows, M.rowptr.p, M.col.p, mval, x, y, ep); };
            if (!dispatch<4, 2>(bk.width, run_w)) run_w(Int<1>{});
          } else launch(bcsr_spmm_kernel<BR, BC, NV, EP, 4>, rowlane_grid(M.n_rows, BR, 4), BLOCK, 0, stream, M.n_rows, M.rowptr.p, M.col.p, mval, x, y, ep);
        };
        ok = dispatch(std::conditional_t<SQ, SquareShapes, RowlaneShapes>{}, key, run);
      } else if constexpr (NV == 1) {
        const int grid = grid_for(M.n_rows * bk.width);
        auto run = [&](auto KEY) {
          constexpr int BR = KEY() / 10, BC = KEY() % 10;
          auto run_g = [&](auto G) { launch(bcsrvec_spmv_kernel<BR, BC, G(), EP>, grid, BLOCK, 0, stream, M.n_rows, M.rowptr.p, M.col.p, mval, x, y, ep); };
          if (!dispatch<2, 4, 8>(bk.width, run_g)) run_g(Int<16>{});
        };
        ok = dispatch(BcsrVecShapes{}, key, run);
      }
      if (!ok) throw Err("unsupported block shape " + std::to_string(M.br) + "x" + std::to_string(M.bc));
    }
  }

  void mult(const DevMatrix& M, const double* x, double* y, const Span sp = Span()) { product<1, EP_MULT>(M, x, y, EpArgs{nullptr, nullptr, nullptr, 0.0, nullptr, 0}, sp); }
  void residual(const DevMatrix& M, const double* x, const double* b, double* r, const Span sp = Span()) { product<1, EP_RES>(M, x, r, EpArgs{b, nullptr, nullptr, 0.0, nullptr, ep_nt & EPF_HOIST}, sp); }
  // the residual a smoother or the cycle forms on its level (update_res, the residual before the restriction): a smoother pass
  void residual_sm(const DevLevel& L, const double* x, const double* b, double* r, const Span sp = Span()) { product<1, EP_RES>(L.A, x, r, EpArgs{b, nullptr, nullptr, 0.0, nullptr, ep_nt & EPF_HOIST}, sp, true); }
  // y = yin + s * M x
  void mult_add(const DevMatrix& M, double s, const double* x, const double* yin, double* y, const Span sp = Span(), bool sm_pass = false) { product<1, EP_AXPY>(M, x, y, EpArgs{nullptr, yin, nullptr, s, nullptr, ep_nt & EPF_HOIST}, sp, sm_pass); }
  // xout = xin + omega * dinv * (b - A xin)
  void jacobi_fused(const DevLevel& L, const double* xin, const double* b, double* xout, const Span sp = Span()) {
    if (xin == xout) throw Err("jacobi_fused: in-place update is not allowed");
    product<1, EP_JAC>(L.A, xin, xout, EpArgs{b, xin, L.dinv.p, L.omega, nullptr, ep_nt}, sp, true);
  }

  // ---- Chebyshev smoother (AMGX_SM_CHEBY) ----
  // xout = (xin ? xin : 0) + c0 * Dinv * v, dout (optional) = the update
  // The block rows [r0, r0 + rows) (default: the owned rows).  A rank-partitioned level may ask for its ghost rows too: v and
  // dinv carry [owned | ghost] entries there.
  void cheb_first(const DevLevel& L, const double* v, const double* xin, double* xout, double* dout, double c0, int64_t r0 = 0, int64_t rows = -1) {
    if (rows < 0) rows = L.n - r0;
    if (r0 < 0 || r0 + rows > L.ncols) throw Err("cheb_first: rows beyond the level's [owned | ghost] range");
    if (rows <= 0) return;
    const int grid = grid_for(rows);
    const int64_t o = r0 * L.bs;
    auto run = [&](auto BS) {
      launch(cheb_first_kernel<BS()>, grid, BLOCK, 0, stream, rows, L.dinv.p + o * L.bs, v + o, xin ? xin + o : nullptr, xout + o, dout ? dout + o : nullptr, c0);
    };
    if (!dispatch<1, 2, 3, 6>(L.bs, run)) throw Err("unsupported block size " + std::to_string(L.bs));
  }
  // one fused step: xout = xin + d_new, d_new = c1 * d_old + c2 * Dinv * (b - A xin); d_old == nullptr: xin; d_new == nullptr: not stored
  // sp: the interior / boundary rows of a rank-partitioned level (formats that are not split run in the boundary part: product())
  void cheb_step(const DevLevel& L, const double* xin, const double* b, double* xout, double c1, double c2, const double* d_old, double* d_new,
                 const Span sp = Span()) {
    if (xin == xout) throw Err("cheb_step: in-place update is not allowed");
    product<1, EP_CHEB>(L.A, xin, xout, EpArgs{b, xin, L.dinv.p, c2, d_new, ep_nt, d_old, c1}, sp, true);
  }
  // One Chebyshev smooth of degree k with the flag contract of base_smooth.  The iterate lives in `src` (x itself or L.tmp, ignored
  // with x_zero) and ends in x; the passes and their operands are cheb_schedule's (cheb_schedule.hpp).  A caller that can choose
  // (post_smooth) puts the iterate at cheb_place(); otherwise one copy moves the result.
  void cheb_smooth(DevLevel& L, const double* src, double* x, const double* b, double* res, bool res_updated, bool update_res, bool x_zero) {
    const int k = L.cheb_degree;
    if (k < 1 || !L.d.p) throw Err("Chebyshev smoother: the level has no coefficients");
    // (single-rank callers only: on a rank-partitioned level the collective drivers of dist.hpp run the schedule around the exchanges)
    if (L.ncols != L.n) throw Err("Chebyshev smoother: a rank-partitioned level is smoothed by the collective cycle (amgx_dist_apply)");
    double* const tmp = L.tmp.p;
    if (!x_zero && src != x && src != tmp) throw Err("Chebyshev smoother: the iterate must live in x or in the level's ping-pong buffer");
    const ChebEntry entry = x_zero ? ChebEntry::ZERO : (res_updated ? ChebEntry::RES_UPDATED : ChebEntry::ITERATE);
    auto first = [&](const double* v, const double* xin, double* xout, double* dout, double c0) { cheb_first(L, v, xin, xout, dout, c0); };
    auto step = [&](const double* xin, double* xout, double c1, double c2, const double* d_old, double* d_new) { cheb_step(L, xin, b, xout, c1, c2, d_old, d_new); };
    const double* cur = cheb_schedule(k, L.cheb_c0, L.cheb_c1, L.cheb_c2, entry, res_updated ? res : b, src, x, tmp, L.d.p, first, step);
    if (cur != x) copy(x, cur, L.len());
    if (update_res) residual_sm(L, x, b, res);
  }

  void zero(double* v, int64_t n) {
    if (n <= 0) return;
    launch(vec_zero_kernel, grid_for((n + 1) / 2), BLOCK, 0, stream, n, v);
  }
  void copy(double* dst, const double* src, int64_t n) {
    if (n <= 0 || dst == src) return;
    launch(vec_copy_kernel, grid_for((n + 1) / 2), BLOCK, 0, stream, n, src, dst);
  }

  // x (+)= omega * dinv * v
  // rows: block rows to process (default: the owned rows; a rank-partitioned level may ask for its ghost rows too)
  void diag_apply(const DevLevel& L, const double* v, double* x, bool add, int64_t rows = -1) {
    if (rows < 0) rows = L.n;
    if (rows == 0) return;
    const int grid = grid_for(rows);
    auto run = [&](auto BS) {
      if (add) launch(diag_apply_kernel<BS(), true>, grid, BLOCK, 0, stream, rows, L.dinv.p, v, x, L.omega);
      else launch(diag_apply_kernel<BS(), false>, grid, BLOCK, 0, stream, rows, L.dinv.p, v, x, L.omega);
    };
    if (!dispatch<1, 2, 3, 6>(L.bs, run)) throw Err("unsupported block size " + std::to_string(L.bs));
  }

  void axpy(int64_t n, double s, const double* x, double* y) {
    if (!n) return;
    launch(axpy_kernel, grid_for(n), BLOCK, 0, stream, n, s, x, y);
  }

  // ------------------------------------------------------------------ the Gauss-Seidel launchers
  // Like product<NV, EP>: NV == 1 names the kernel of kernels.hpp, NV == 2, 4 its form on interleaved vectors (multi_kernels.hpp;
  // AMGX_MULTI_FUSE_GS and AMGX_MULTI_FUSE_GS_BLOCK).  Colour order, grids, lane and size lists and the checks
  // on the iterate are written once; what the widths do not share is stated once too, as a fact about NV:
  //   units        NV > 1 sweeps whole levels (gs_units), as product<NV > 1> takes no Span
  //   images       every width reads the single-precision images of a level that has them (gs_prec, gs_view; scalar levels: sgs_image):
  //                the six NV sweep kernels are built on float too.  NV > 1 reaches such a level only where the call
  //                carries AMGX_MULTI_FUSE_F32 and multi_f32_ok holds.  NV > 1 reads BSELL images in the plain view, one vector in the
  //                view of knobs.bsell_xmode
  //   block size   a size the BSELL kernels are not listed for takes the 2 x 2 kernel on one vector and an fp64 image, and is an error
  //                on NV > 1 and on float images (gs_bsell_size)
  //   hybrid form  the local-window image and the mid-width kernel of gsb_sweep are built for one vector (GSB_FORMS there)
  //   LDS          bgsb_sweep asks for multi_block_sweep_lds(L, NV); NV > 1 refuses what exceeds 64 KB
  // The roctx markers cover every width (gs_range_name: literals, no string per call).
  // And, in the routing below: the split identity (split_identity), the epilogue arguments (residual_after_zero) and the aggregate
  // blocks, which have no NV form (sweep).
  template <class F>
  static void gs_lanes(int lanes, F&& run) { if (!dispatch<1, 2, 4, 8>(lanes, run)) run(Int<16>{}); }      // any other lane count: the 16-lane kernel
  // the units [beg, end) among the n of a level that a sweep covers; false: none
  template <int NV>
  static bool gs_units(const Units u, int n, int& beg, int& end) {
    if (NV > 1 && (u.beg != 0 || u.end >= 0)) throw Err("multi-vector Gauss-Seidel: the sweeps cover whole levels");
    beg = u.beg;
    end = (u.end < 0 || u.end > n) ? n : u.end;
    return end > beg;
  }
  // The BSELL images that the sweeps of a Gauss-Seidel block level read: the single-precision ones where mat_f32_image gave the level
  // the images (DevLevel::gs32), otherwise the fp64 ones.  gs_prec: run(value type); gs_view<NV, T>: the view of image M.
  // Nothing else is decided at launch time.
  template <int NV, class F>
  static void gs_prec(const DevLevel& L, F&& run) {
    if (L.gs32) { run(float{}); return; }
    run(double{});
  }
  template <int NV, class T>
  BSellMatT<T> gs_view(const DevMatrix& M) const {
    const int xmode = NV == 1 ? knobs.bsell_xmode : 0;       // (the gather variants rearrange loads that the NV > 1 kernels do not have)
    if constexpr (std::is_same_v<T, float>) {
      if (M.val32.n != M.bsell.val.n) throw Err("single-precision Gauss-Seidel images: a sweep image has no float twin");
      return M.bsell.view32(M.val32.p, xmode);
    } else return M.bsell.view(xmode);
  }
  // The sliced-ELL images that the sweeps of a SCALAR Gauss-Seidel level read: run(view) gets the float view on a level with
  // single-precision images (DevLevel::sgs32; NV > 1: 5.22), otherwise the fp64 one.  An fp64 view of released values
  // is an error here, never a null pointer in a kernel.
  template <int NV, class F>
  static void sgs_image(const DevLevel& L, const DevMatrix::Sell& S, F&& run) {
    if (L.sgs32) {
      if (!S.val32.p && S.val.p) throw Err("single-precision Gauss-Seidel images: a sweep image has no float twin");
      run(S.view32());
      return;
    }
    if (!S.val.p && S.val32.p) throw Err("Gauss-Seidel sweep: the fp64 values of this image were released (single-precision Gauss-Seidel images); only the single-vector passes of the level read it");
    run(S.view());
  }
  // the block sizes of the BSELL colour and upper-residual kernels
  template <int NV, class T, class F>
  static void gs_bsell_size(int bs, F&& run) {
    if (dispatch<6, 3, 2>(bs, run)) return;
    if (NV > 1) throw Err("multi-vector Gauss-Seidel: unsupported block size");
    if (std::is_same_v<T, float>) throw Err("single-precision Gauss-Seidel images: unsupported block size " + std::to_string(bs));
    run(Int<2>{});                                             // one vector, fp64 image, any other block size: the 2 x 2 kernel
  }

  // one multicolour GS sweep (RHS form), in place, one launch per colour; forward: colours ascending, backward: descending
  // u: only the colours [beg, end) -- the stages of the hybrid smoother on rank-partitioned levels are colour ranges (dist.hpp)
  // lower_only: over the couplings to lower colours (the sweep from zero of a level with the split images)
  template <int NV = 1>
  void gs_sweep(const DevLevel& L, int dir, double* x, const double* b, bool lower_only = false, const Units u = Units()) {
    Range rg(gs_range_name(L.bs));
    const DevGS& g = L.gs;
    const DevMatrix::Sell& copy = (lower_only && g.has_split) ? g.lower : g.sell;
    if (L.paths.hybrid()) throw Err("gs_sweep: the level uses the block-hybrid form");
    if (g.n_colors == 0 && L.n > 0) throw Err("Gauss-Seidel requested but the level has no colouring");
    int cbeg, cend;
    gs_units<NV>(u, g.n_colors, cbeg, cend);
    for (int q = cbeg; q < cend; ++q) {
      const int c = dir == 0 ? q : cend - 1 - (q - cbeg);
      if (L.bs == 1) {
        const int s0 = g.color_slice_ptr[c], s1 = g.color_slice_ptr[c + 1];
        if (s1 == s0) continue;
        sgs_image<NV>(L, copy, [&](auto M) {
          using V = std::remove_const_t<std::remove_pointer_t<decltype(M.val)>>;       // double / float
          gs_lanes(g.lanes, [&](auto GG) {
            if constexpr (NV == 1) launch(gs_color_kernel<GG(), V>, wave_grid(s1 - s0), BLOCK, 0, stream, s0, s1, M, g.rowid.p, L.dinv.p, b, x);
            else launch(gs_color_nv_kernel<GG(), NV, V>, wave_grid(s1 - s0), BLOCK, 0, stream, s0, s1, M, g.rowid.p, L.dinv.p, b, x);
          });
        });
      } else if (g.bsell_ok) {
        const int s0 = g.color_slice_ptr[c], s1 = g.color_slice_ptr[c + 1];
        if (s1 == s0) continue;
        const DevMatrix& CM = (lower_only && g.bsplit) ? g.blower : g.bcopy;
        gs_prec<NV>(L, [&](auto prec) {
          using T = decltype(prec);                                   // double / float
          const BSellMatT<T> BM = gs_view<NV, T>(CM);
          gs_bsell_size<NV, T>(L.bs, [&](auto BS) {
            if constexpr (NV == 1) launch(bgs_bsell_color_kernel<BS(), T>, wave_grid(s1 - s0), BLOCK, 0, stream, s0, s1, BM, g.rowid.p, L.dinv.p, b, x);
            else launch(bgs_bsell_color_nv_kernel<BS(), NV, T>, wave_grid(s1 - s0), BLOCK, 0, stream, s0, s1, BM, g.rowid.p, L.dinv.p, b, x);
          });
        });
      } else {
        const int r0 = g.color_row_ptr[c], r1 = g.color_row_ptr[c + 1];
        if (r1 == r0) continue;
        const double avg = L.A.n_rows ? (double)L.A.nnz / (double)L.A.n_rows : 0.0;
        const int W = bgs_rowlist_w(avg, r1 - r0);
        const int grid = rowlane_grid(r1 - r0, L.bs, W);
        auto run = [&](auto BS) {
          auto run_w = [&](auto WW) {
            if constexpr (NV == 1) launch(bgs_color_kernel<BS(), WW()>, grid, BLOCK, 0, stream, r0, r1, g.rowlist.p, L.A.rowptr.p, L.A.col.p, L.A.val.p, L.dinv.p, b, x);
            else launch(bgs_color_nv_kernel<BS(), WW(), NV>, grid, BLOCK, 0, stream, r0, r1, g.rowlist.p, L.A.rowptr.p, L.A.col.p, L.A.val.p, L.dinv.p, b, x);
          };
          if (!dispatch<8, 4, 2>(W, run_w)) run_w(Int<1>{});
        };
        if (!dispatch<2, 3, 6>(L.bs, run)) throw Err("unsupported block size for GS");
      }
    }
  }
  // r = -(U x) right after the multicolour sweep from zero over the lower couplings, one launch over all colours: b - L x - D x = 0
  // on every swept row (r on non-free rows is not needed: their prolongation rows are empty).  Scalar levels: `upper`; block levels
  // in the BSELL form: r_B = -(U x)_B from `bupper`.
  template <int NV = 1>
  void gs_upper_residual(const DevLevel& L, const double* x, double* r) {
    const DevGS& g = L.gs;
    const int ns = L.bs == 1 ? g.n_slices_total : g.bupper.n_slices;
    if (ns <= 0) return;
    if (L.bs == 1) {
      sgs_image<NV>(L, g.upper, [&](auto M) {
        using V = std::remove_const_t<std::remove_pointer_t<decltype(M.val)>>;         // double / float
        gs_lanes(g.lanes, [&](auto GG) {
          if constexpr (NV == 1) launch(gs_upper_residual_kernel<GG(), V>, wave_grid(ns), BLOCK, 0, stream, ns, M, g.rowid.p, x, r);
          else launch(gs_upper_residual_nv_kernel<GG(), NV, V>, wave_grid(ns), BLOCK, 0, stream, ns, M, g.rowid.p, x, r);
        });
      });
      return;
    }
    gs_prec<NV>(L, [&](auto prec) {
      using T = decltype(prec);                                       // double / float
      const BSellMatT<T> UM = gs_view<NV, T>(g.bupper);
      gs_bsell_size<NV, T>(L.bs, [&](auto BS) {
        if constexpr (NV == 1) launch(bgs_bsell_upper_residual_kernel<BS(), T>, wave_grid(ns), BLOCK, 0, stream, ns, UM, g.rowid.p, x, r);
        else launch(bgs_bsell_upper_residual_nv_kernel<BS(), NV, T>, wave_grid(ns), BLOCK, 0, stream, ns, UM, g.rowid.p, x, r);
      });
    });
  }

  // one block-hybrid Gauss-Seidel sweep (gsb_sweep_kernel): ONE launch, out of place; xin == nullptr: sweep from x = 0
  // u: only the blocks [beg, end): blocks are independent of each other within a sweep, so the rank-partitioned driver sweeps its
  // boundary and interior blocks in separate launches around the halo exchange
  // The image follows from the call: from zero on a level with the split `lowin` (the narrow form where gsb.narrow holds), otherwise
  // `full` (one vector: or its local-window form).
  template <int NV = 1>
  void gsb_sweep(const DevLevel& L, int dir, const double* xin, double* xout, const double* b, const Units u = Units()) {
    Range rg(gs_range_name(1));
    constexpr bool GSB_FORMS = NV == 1;      // the local-window image and the mid-width kernel exist
    const DevGSB& g = L.gsb;
    int blk0, blk1;
    if (!gs_units<NV>(u, g.n_blocks, blk0, blk1)) return;
    if (xin == xout) throw Err("block-hybrid Gauss-Seidel sweeps are out of place");
    const bool fz = xin == nullptr;
    const bool lowin = fz && L.paths.zero_split;
    const bool lw = GSB_FORMS && !fz && g.lw;
    GsbArgs a{g.rowid.p, g.slotcolor.p, L.dinv.p, b, g.n_colors, dir, lw ? g.flw_cptr.p : nullptr, lw ? g.flw_ccol.p : nullptr};
    const DevMatrix::Sell& image = lw ? g.fullLW : lowin ? g.lowin : g.full;
    const bool narrow = lowin && g.narrow;
    const bool mid = GSB_FORMS && !fz && g.mid;
    // <workgroup size, lanes per row, from zero, entries per lane and pass, local-window image, value type>; the mid-width and
    // local-window forms exist for more than one lane per row only
    sgs_image<NV>(L, image, [&](auto M) {
      using V = std::remove_const_t<std::remove_pointer_t<decltype(M.val)>>;             // double / float
      auto run = [&](auto TT) {
        gs_lanes(g.G, [&](auto GG) {
          auto sweep = [&](auto ZZ, auto WW, auto LW) {
            if constexpr (NV == 1) launch(gsb_sweep_kernel<TT(), GG(), ZZ(), WW(), LW(), V>, blk1 - blk0, TT(), 0, stream, L.n, blk0, M, a, xin, xout);
            else launch(gsb_sweep_nv_kernel<TT(), GG(), ZZ(), WW(), NV, V>, blk1 - blk0, TT(), 0, stream, L.n, M, a, xin, xout);    // (whole level: no first block)
          };
          constexpr std::false_type no{};
          constexpr std::true_type yes{};
          if (narrow) return sweep(yes, Int<2>{}, no);
          if (fz) return sweep(yes, Int<GSB_WP>{}, no);
          if constexpr (GSB_FORMS && GG() > 1) {
            if (lw && mid) return sweep(no, Int<5>{}, yes);
            if (lw) return sweep(no, Int<GSB_WP>{}, yes);
            if (mid) return sweep(no, Int<5>{}, no);
          }
          sweep(no, Int<GSB_WP>{}, no);
        });
      };
      if (!dispatch<256, 512>(g.TH, run)) run(Int<1024>{});            // any other workgroup size: 1024
    });
  }

  // one block-hybrid Gauss-Seidel sweep on a square-block level (bgsb_sweep_kernel).  Hybrid form: ONE launch, out of place
  // (xin == nullptr: from x = 0); u: the sweep blocks [beg, end) only (rank-partitioned levels: boundary blocks before, interior
  // blocks beside the exchange).  Block-coloured form: whole level, in place, one launch per block colour.
  template <int NV = 1>
  void bgsb_sweep(const DevLevel& L, int dir, const double* xin, double* xout, const double* b, const Units u = Units()) {
    Range rg(gs_range_name(L.bs));
    const DevBGSB& g = L.bgsb;
    const size_t lds = multi_block_sweep_lds(L, NV);
    if (NV > 1 && lds > (size_t)64 * 1024) throw Err("multi-vector Gauss-Seidel: sweep block too large");
    // the images: fp64, or the single-precision ones of a level that has them (gs_prec).  IN / OTH -- forward: colour phases over
    // the couplings to lower colours, the upper ones stream with the sweep-start values; backward: reversed.  OFF: `off`, or `offlo`
    // for the block-coloured sweep from zero
    auto sweep = [&](auto MODE, const DevMatrix& off, const int32_t* list, int b0, int nb, const double* x0) {
      gs_prec<NV>(L, [&](auto prec) {
        using T = decltype(prec);                                     // double / float
        const BSellMatT<T> OFF = gs_view<NV, T>(off), IN = gs_view<NV, T>(dir == 0 ? g.in : g.upin), OTH = gs_view<NV, T>(dir == 0 ? g.upin : g.in);
        auto run = [&](auto BS) {
          if constexpr (NV == 1)
            launch(bgsb_sweep_kernel<BS(), MODE(), T>, nb, BLOCK, lds, stream, g.BB, b0, list, g.blk_ptr.p, g.blk_rows.p, OFF, g.off_ptr.p, IN, OTH,
                   g.in_ptr.p, g.in_row.p, g.n_colors, dir, L.dinv.p, b, x0, xout);
          else
            launch(bgsb_sweep_nv_kernel<BS(), MODE(), NV, T>, nb, BLOCK, lds, stream, g.BB, b0, list, g.blk_ptr.p, g.blk_rows.p, OFF, g.off_ptr.p, IN, OTH,
                   g.in_ptr.p, g.in_row.p, g.n_colors, dir, L.dinv.p, b, x0, xout);
        };
        if (!dispatch<2, 3, 6>(L.bs, run)) throw Err("block-hybrid Gauss-Seidel: unsupported block size");
      });
    };
    const bool fz = xin == nullptr;
    int blk0, blk1;
    const bool some = gs_units<NV>(u, g.n_blocks, blk0, blk1);
    if (g.bc) {
      // from zero the first colour reads nothing outside its blocks, the later ones the finished blocks of lower colours through
      // `offlo` (which exists with the split)
      if (u.beg != 0 || (u.end >= 0 && u.end != g.n_blocks)) throw Err("block-coloured Gauss-Seidel sweeps cover the whole level");
      if (!fz && xin != xout) throw Err("block-coloured Gauss-Seidel sweeps work in place");
      if (fz && dir != 0) throw Err("block-coloured Gauss-Seidel: the sweep from zero is a forward sweep");
      if (fz && !L.paths.zero_split) throw Err("block-coloured Gauss-Seidel from zero needs the split images (zero x and sweep in place instead)");
      for (int q = 0; q < g.n_bcolors; ++q) {
        const int c = dir ? g.n_bcolors - 1 - q : q;
        const int b0 = g.bc_ptr[c], nb = g.bc_ptr[c + 1] - b0;
        if (nb <= 0) continue;
        if (!fz) sweep(Int<0>{}, g.off, g.blk_list.p, b0, nb, xout);
        else if (q == 0) sweep(Int<1>{}, g.offlo, g.blk_list.p, b0, nb, nullptr);
        else sweep(Int<2>{}, g.offlo, g.blk_list.p, b0, nb, xout);
      }
      return;
    }
    if (!some) return;
    if (xin == xout) throw Err("block-hybrid Gauss-Seidel sweeps are out of place");
    if (fz) sweep(Int<1>{}, g.off, nullptr, blk0, blk1 - blk0, xin);
    else sweep(Int<0>{}, g.off, nullptr, blk0, blk1 - blk0, xin);
  }

  // ---- which levels have the sweeps on NV = 2, 4 vectors is asked here, next to the launchers, and nowhere else (through
  // Multi::facts: the rule of multi_rule.hpp, amgx_smooth_multi).  Scalar levels (AMGX_MULTI_FUSE_GS):
  // f32: the call carries AMGX_MULTI_FUSE_F32; without it a level with single-precision images has no NV sweep
  bool multi_sweep_ok(const DevLevel& L, bool f32 = false) const {
    if (L.sm_type != AMGX_SM_GS || L.bs != 1 || L.n != L.ncols || !L.paths.plain) return false;
    if ((L.sgs32 || L.sgs32_wide) && !(f32 && multi_f32_ok(L))) return false;       // single-precision images
    return L.paths.sweep == SWEEP_GSB || L.paths.sweep == SWEEP_MC;
  }
  // ... square-block levels (AMGX_MULTI_FUSE_GS_BLOCK; multi_sweep_ok keeps the answer of AMGX_MULTI_FUSE_GS)
  bool multi_block_sweep_ok(const DevLevel& L, bool f32 = false) const {
    if (L.sm_type != AMGX_SM_GS || (L.bs != 2 && L.bs != 3 && L.bs != 6) || L.n != L.ncols || !L.paths.plain) return false;
    if ((L.gs32 || L.gs32_wide) && !(f32 && multi_f32_ok(L))) return false;         // single-precision images
    switch (L.paths.sweep) {
      case SWEEP_BGSB: case SWEEP_BGSB_BC: case SWEEP_MC_BSELL: case SWEEP_MC_ROWLIST: return true;
      default: return false;
    }
  }
  // The float question (AMGX_MULTI_FUSE_F32): the level has single-precision Gauss-Seidel images (or is their
  // AMGX_GS_F32_WIDE twin) and every image its fused passes read -- the sweeps, the sweep from zero, the residual after it -- has a kernel
  // on NV vectors for the array the single-vector pass reads: the float array, on the twin the rounded values at fp64 width.  So a
  // fused pass reads the values of the single-vector pass, image by image.  Scalar levels: the sweep images are sliced-ELL with a float
  // array; `rest` is plain or windowed sliced-ELL with a float array, or CSR-vector (a badly padded remainder) with the rounded values
  // at fp64 width in place; A of a level without the split is plain sliced-ELL with a float array, or keeps the rounded values in
  // val64r.  Block levels: every sweep image is BSELL with a float array; A is BSELL with one, or block CSR with val64r.  Anything
  // else -- an image without the array its single-vector pass reads -- does not qualify.
  bool multi_f32_ok(const DevLevel& L) const {
    const LevelPaths& P = L.paths;
    if (L.bs == 1) {
      if (!(L.sgs32 || L.sgs32_wide) || (P.sweep != SWEEP_GSB && P.sweep != SWEEP_MC)) return false;
      const bool wide = L.sgs32_wide;
      auto sell = [&](const DevMatrix::Sell& S) { return S.val.n + S.val32.n == 0 || (wide ? S.val.p != nullptr : S.val32.p != nullptr); };
      auto a_ok = [&] { return multi_scalar_ok(L.A) && (wide ? L.A.val64r.p != nullptr : (L.A.has32() ? L.A.fmt == FMT_SELL && !L.A.sell.win : L.A.val64r.p != nullptr)); };
      if (P.sweep == SWEEP_GSB) {
        const DevGSB& g = L.gsb;
        if (!sell(g.full)) return false;
        if (!P.zero_split) return a_ok();
        if (!sell(g.lowin) || !multi_scalar_ok(g.rest)) return false;
        if (g.rest.fmt != FMT_SELL) return g.rest.val.p != nullptr && !g.rest.has32();
        return g.rest.sell.val.n + g.rest.val32.n == 0 || (wide ? g.rest.sell.val.p != nullptr : g.rest.has32());
      }
      const DevGS& g = L.gs;
      if (!sell(g.sell)) return false;
      if (!P.zero_split) return a_ok();
      return sell(g.lower) && sell(g.upper);
    }
    if (!(L.gs32 || L.gs32_wide) || (P.sweep != SWEEP_BGSB && P.sweep != SWEEP_BGSB_BC && P.sweep != SWEEP_MC_BSELL)) return false;
    const bool wide = L.gs32_wide;
    auto img = [&](const DevMatrix& M) { return M.empty() || (M.fmt == FMT_BSELL && (M.bsell.val.n == 0 || wide || M.val32.n == M.bsell.val.n)); };
    auto a_ok = [&] { return L.A.fmt == FMT_BSELL ? (wide ? L.A.val64r.p != nullptr : L.A.has32()) : L.A.val64r.p != nullptr; };
    if (P.bgsb()) {
      const DevBGSB& g = L.bgsb;
      if (!img(g.off) || !img(g.in) || !img(g.upin)) return false;
      if (!P.zero_split) return a_ok();
      return img(g.offlo) && img(g.rest) && split_identity(L, 2);
    }
    const DevGS& g = L.gs;
    if (!img(g.bcopy)) return false;
    if (!P.zero_split) return a_ok();
    return img(g.blower) && img(g.bupper);
  }
  // dynamic LDS of bgsb_sweep: x and b' of a sweep block on nv (interleaved) vectors, and its row ids
  static size_t multi_block_sweep_lds(const DevLevel& L, int nv) {
    return (size_t)2 * L.bgsb.BB * L.bs * nv * sizeof(double) + (size_t)L.bgsb.BB * sizeof(int);
  }
  // ... which has to fit the 64 KB a launch gets without asking at the widest group (only AMGX_BGSB_ROWS makes blocks that do not)
  bool multi_block_sweep_fits(const DevLevel& L) const { return !L.paths.bgsb() || multi_block_sweep_lds(L, 4) <= (size_t)64 * 1024; }

  // one block Gauss-Seidel sweep: colours of the block graph ascending (forward) or descending (backward)
  void bgs_sweep(const DevLevel& L, int dir, double* x, const double* b, int cbeg = 0, int cend = -1) {
    const DevBGS& g = L.bgs;
    if (g.n_colors == 0 && L.n > 0 && g.block_ptr.n > 1) throw Err("block Gauss-Seidel requested but the level has no block colouring");
    if (cend < 0 || cend > g.n_colors) cend = g.n_colors;
    for (int q = cbeg; q < cend; ++q) {
      const int c = dir == 0 ? q : cend - 1 - (q - cbeg);
      const int b0 = g.color_ptr[c], b1 = g.color_ptr[c + 1];
      if (b1 == b0) continue;
      const double avg = L.A.n_rows ? (double)L.A.nnz / (double)L.A.n_rows : 0.0;
      const BgsShape shape = bgs_block_shape(avg, g.max_m);
      const int G = shape.G, TH = shape.TH;
      auto run = [&](auto BS) {
        auto block = [&](auto TT, auto GG) {
          launch(bgs_block_kernel<BS(), TT(), GG()>, b1 - b0, TT(), 0, stream, b0, g.blocklist.p, g.block_ptr.p, g.block_rows.p, g.rowptr.p, g.col.p, g.val.p,
                 g.dinv_ptr.p, g.dinv.p, b, x);
        };
        if (G == 4 && TH == 256) block(Int<256>{}, Int<4>{});
        else if (G == 4 && TH == 512) block(Int<512>{}, Int<4>{});
        else if (G == 4) block(Int<1024>{}, Int<4>{});
        else if (G == 8) block(Int<1024>{}, Int<8>{});          // (no <512, 8>: unreachable, see bgs_block_shape)
        else block(Int<1024>{}, Int<16>{});
      };
      if (!dispatch<1, 2, 3, 6>(L.bs, run)) throw Err("unsupported block size for block Gauss-Seidel");
    }
  }

  // ---- the Gauss-Seidel step of a level on NV vectors: these functions (and residual_restrict_after_zero below) are the only ones
  //      that switch over LevelPaths::sweep; the smoothers, the cycles, the rank-partitioned drivers (dist.hpp) and the multi-vector
  //      path (multi.hpp, under its width dispatch) call them
  // One sweep on the iterate `cur`; entries outside the swept units keep the values of `cur`.  Returns the buffer that holds the
  // result: `cur` for the in-place forms (oth may be null), `oth` for the out-of-place ones.
  template <int NV = 1>
  double* sweep(const DevLevel& L, int dir, double* cur, double* oth, const double* b, const Units u = Units()) {
    switch (L.paths.sweep) {
      case SWEEP_GSB: gsb_sweep<NV>(L, dir, cur, oth, b, u); return oth;
      case SWEEP_BGSB: bgsb_sweep<NV>(L, dir, cur, oth, b, u); return oth;
      case SWEEP_BGSB_BC: bgsb_sweep<NV>(L, dir, cur, cur, b, u); return cur;
      case SWEEP_BGS:
        if constexpr (NV > 1) throw Err("multi-vector Gauss-Seidel: aggregate blocks have no multi-vector form");
        else { bgs_sweep(L, dir, cur, b, u.beg, u.end); return cur; }
      default: gs_sweep<NV>(L, dir, cur, b, false, u); return cur;
    }
  }
  // r = b - A x after the sweep from zero comes from the identity of the level's split images.  One vector: wherever the level has
  // them.  NV > 1: where the identity is a product, only where product<NV> serves the `rest` image; otherwise r = b - A x from A
  // (the sweep from zero still runs over the split image).  The multicolour identities have kernels of their own for every NV.
  static bool split_identity(const DevLevel& L, int nv) {
    const LevelPaths& P = L.paths;
    if (nv == 1 || !P.zero_split) return P.zero_split;
    if (P.bgsb()) return multi_level_ok(L.bgsb.rest) && L.bgsb.rest.br == L.bs;
    return P.sweep != SWEEP_GSB || multi_scalar_ok(L.gsb.rest);
  }
  // The forward sweep from x = 0.  With LevelPaths::zero_split it runs over the couplings to lower colours only -- everything
  // else multiplies zeros -- and residual_after_zero gets r from the rest, so that A is read once in total.  r: the vector
  // residual_after_zero will fill; the multicolour identity writes swept rows only, so r is cleared here, beside x.
  template <int NV = 1>
  void sweep_from_zero(const DevLevel& L, double* x, const double* b, double* r, const Units u = Units()) {
    const LevelPaths& P = L.paths;
    if (!P.in_place) { sweep<NV>(L, 0, nullptr, x, b, u); return; }    // (out of place: xin == nullptr is the sweep from zero)
    if (P.sweep == SWEEP_BGSB_BC && P.zero_split) { bgsb_sweep<NV>(L, 0, nullptr, x, b, u); return; }
    zero(x, L.len() * NV);
    if (!P.zero_split) { sweep<NV>(L, 0, x, nullptr, b, u); return; }
    if (!r) throw Err("sweep_from_zero: the split multicolour form clears the residual vector too");
    zero(r, L.len() * NV);
    gs_sweep<NV>(L, 0, x, b, true, u);
  }
  // r = b - A x right after sweep_from_zero(L, x, b, r), by the identity the level's images allow (x may carry ghost entries)
  // The products are passes of the smoother on the level: they read the single-precision image of `rest` on a level with such
  // Gauss-Seidel images, on every width.  One vector hoists its epilogue loads where ep_nt says so; NV > 1 passes no epilogue flags.
  template <int NV = 1>
  void residual_after_zero(const DevLevel& L, const double* x, const double* b, double* r) {
    const int nt = NV == 1 ? ep_nt & EPF_HOIST : 0;
    if (!split_identity(L, NV)) { product<NV, EP_RES>(L.A, x, r, EpArgs{b, nullptr, nullptr, 0.0, nullptr, nt}, Span(), true); return; }
    switch (L.paths.sweep) {
      case SWEEP_GSB:
        // inside a block only couplings to lower colours contributed; (b - L_in x)_k = x_k / dinv_k on every swept row, hence
        // r = b - A x = (1/dinv - a_kk) .* x - (A - L_in - D) x = c .* x - rest x
        product<NV, EP_CRES>(L.gsb.rest, x, r, EpArgs{x, nullptr, L.gsb.cvec.p, 0.0, nullptr, nt}, Span(), L.sgs32);
        return;
      case SWEEP_BGSB: case SWEEP_BGSB_BC:                                          // r = rest x (see DevBGSB)
        product<NV, EP_MULT>(L.bgsb.rest, x, r, EpArgs{nullptr, nullptr, nullptr, 0.0, nullptr, 0}, Span(), L.gs32);
        return;
      case SWEEP_MC: case SWEEP_MC_BSELL: gs_upper_residual<NV>(L, x, r); return;   // r = -(U x) on the swept rows
      default: throw Err("residual_after_zero: the level's sweep form has no split identity");
    }
  }

  void coarse_solve(const double* rhs, double* x) {
    Range rg("coarse inv");
    const DevLevel& L = lev.back();
    if (clev != AMGX_CLEV_INV || coarse_n == 0) { zero(x, L.len()); return; }   // amg_matrix.cpp:242-246
    const int grid = wave_grid(coarse_n);
    if (coarse_ld != coarse_n) launch(dense_op_gemv_kernel, grid, BLOCK, 0, stream, (int)coarse_n, (int)coarse_ld, coarse_inv.p, rhs, x);
    else launch(dense_gemv_kernel, grid, BLOCK, 0, stream, (int)coarse_n, coarse_inv.p, rhs, x);
  }

  // adds the partial sums of the chunk-local restriction of level l (restrict_chunk_kernel and the fused down kernels leave
  // them in R.part) into the right-hand side of level l + 1
  void restrict_sum(int l, const DevRestrict& R, double* b_coarse) {
    launch(restrict_sum_kernel, grid_for((lev[l + 1].n + RSUM_R - 1) / RSUM_R * RSUM_G), BLOCK, 0, stream, lev[l + 1].n, R.optr.p, R.oidx.p, R.part.p, b_coarse);
  }

  void transfer_f2c(int l, const double* xf, double* xc) {                                               // dof_map.cpp:636-654
    Range rg("ProlMap::TransferF2C");
    const DevRestrict& R = lev[l].R;
    if (R.empty()) { mult(lev[l].PT, xf, xc); return; }
    launch(restrict_chunk_kernel, R.n_chunks, BLOCK, 0, stream, lev[l].n, R.chunk_slot.p, R.slot_ptr.p, R.w.p, R.fi.p, xf, R.part.p, R.dest.p);
    restrict_sum(l, R, xc);
  }
  void add_c2f(int l, double fac, double* xf, const double* xc) { Range rg("ProlMap::TransferC2F"); mult_add(lev[l].P, fac, xc, xf, xf); }   // dof_map.cpp:697-709

  // ------------------------------------------------------------------ smoothers (flag contract: base_smoother.hpp:68-112)
  void base_smooth(DevLevel& L, int dir, double* x, const double* b, double* res, bool res_updated, bool update_res, bool x_zero) {
    if (L.sm_type == AMGX_SM_JACOBI) {
      // RichardsonSmoother::Smooth, base_smoother.cpp:61-74 (SmoothBack identical)
      if (!res_updated && x_zero) diag_apply(L, b, x, true);
      else {
        // (the residual inside the Jacobi step is a pass of the smoother: it reads the level's single-precision image)
        if (!res_updated) residual_sm(L, x, b, res);
        diag_apply(L, res, x, true);
      }
      // update_res: inside pre-smoothing from zero (pre_smooth: the residual that goes to the restriction, |r| ~ |b|) a pass of the
      // level as well; anywhere else (the second visit of a W / BS cycle, amgx_smooth) the residual of an iterate that a further
      // correction uses, which reads the fp64 A for the reason given at the Gauss-Seidel branch below
      if (update_res) { if (pre_from_zero) residual_sm(L, x, b, res); else residual(L.A, x, b, res); }
    } else if (L.sm_type == AMGX_SM_CHEBY) {
      // symmetric polynomial smoother: Smooth and SmoothBack are the same operation
      cheb_smooth(L, x, x, b, res, res_updated, update_res, x_zero);
    } else {
      // GSS3::Smooth / SmoothBack (gssmoother.cpp:350-398), BSmoother::Smooth / SmoothBack (block_gssmoother.cpp:434-498).  The
      // reference keeps the residual current with row-transpose scatters (RES form); for symmetric A the gather (RHS) form
      // followed by one residual SpMV gives the same x and res, and it has no write conflicts on a GPU.
      if (L.paths.in_place) sweep(L, dir, x, nullptr, b);
      else {
        copy(L.tmp.p, x, L.ext_len());       // (out of place: the off-block values are those from the start of the sweep)
        sweep(L, dir, L.tmp.p, x, b);
      }
      // The residual of an iterate that a further correction will use (W / BS cycles, ProxySmoother chains, amgx_smooth) reads the fp64
      // A also on a level with single-precision Gauss-Seidel images: x is close to the solution there, b - A x cancels,
      // and a residual formed with the rounded A would steer the next correction towards the solution of the ROUNDED system -- a shift of
      // cond(A) * 6e-8 in the cycle's result (measured: 3.4e-6 in the W-cycle of a 40 x 36 elasticity grid against 5e-8 in its V-cycle).
      // The residual right after the sweep from zero (residual_after_zero: |r| ~ |b|, nothing cancels) reads the float images.
      // A scalar level with single-precision images follows 5.20: inside pre-smoothing from zero the residual goes to
      // the restriction (|r| ~ |b|) and is a pass of the level, on the image the sweeps read
      if (update_res) { if (pre_from_zero && (L.sgs32 || L.sgs32_wide)) residual_sm(L, x, b, res); else residual(L.A, x, b, res); }
    }
  }

  bool pre_from_zero = false;           // base_smooth runs inside pre_smooth's step chain from x = 0 (see update_res above)
  void smooth_symm(DevLevel& L, double* x, const double* b, double* res, bool ru, bool ur, bool xz) {
    base_smooth(L, 0, x, b, res, ru, ur, xz);
    base_smooth(L, 1, x, b, res, ur, ur, false);
  }

  // ProxySmoother (base_smoother.hpp:169-229), present iff sm_symm || sm_steps > 1 (amg_pc.cpp:1079-1082)
  void level_smooth(DevLevel& L, int dir, double* x, const double* b, double* res, bool ru, bool ur, bool xz) {
    const int k = std::max(1, L.sm_steps);
    if (!L.sm_symm && k == 1) { base_smooth(L, dir, x, b, res, ru, ur, xz); return; }
    if (L.sm_symm) {
      smooth_symm(L, x, b, res, ru, ur, xz);
      for (int j = 1; j < k; ++j) smooth_symm(L, x, b, res, ur, ur, false);
    } else {
      base_smooth(L, dir, x, b, res, ru, ur, xz);
      for (int j = 1; j < k; ++j) base_smooth(L, dir, x, b, res, ur, ur, false);
    }
  }

  // (accessors of what resolve_paths decided: multi.hpp and dist.hpp ask through the handle)
  bool plain(const DevLevel& L) const { return L.paths.plain; }
  bool folded(const DevLevel& L) const { return L.paths.folded; }
  // HIP events of amgx_time_op (ops 8 and 9) around the launches of `body`
  template <class F>
  void probed(bool on, F&& body) {
    if (on) HIPCHK(hipEventRecord(probe_e0, stream));
    body();
    if (on) HIPCHK(hipEventRecord(probe_e1, stream));
  }
  // the life of the probe events (amgx_time_op ops 8 / 9, amgx_dist_time_kernel): both exist while the scope does; the cycle
  // records them once `probe_level` is set (after the warm-up), and leaving the scope by any path switches the probe off
  struct ProbeScope {
    Handle& h;
    ProbeScope(Handle& hh, int kind) : h(hh) {
      h.probe_kind = kind;
      HIPCHK(hipEventCreate(&h.probe_e0));
      const hipError_t e = hipEventCreate(&h.probe_e1);
      if (e != hipSuccess) { release(); HIPCHK(e); }
    }
    ProbeScope(const ProbeScope&) = delete;
    ~ProbeScope() { release(); }
    void release() {
      h.probe_level = -1;
      if (h.probe_e0) (void)hipEventDestroy(h.probe_e0);
      if (h.probe_e1) (void)hipEventDestroy(h.probe_e1);
      h.probe_e0 = h.probe_e1 = nullptr;
    }
    float elapsed_ms() const { float ms = 0; HIPCHK(hipEventElapsedTime(&ms, h.probe_e0, h.probe_e1)); return ms; }
  };

  // pre-smoothing step of the cycles: x = 0; r = b; Smooth(x, b, r, 1, 1, 1)   (amg_matrix.cpp:193-206)
  // fold (only with folded(L)): x receives z = x + omega*Dinv*r, to be completed by post_smooth(..., fold = true)
  void pre_smooth(DevLevel& L, double* x, const double* b, double* r, bool fold = false, const Span sp = Span()) {
    const LevelPaths& P = L.paths;
    const bool jacobi = P.plain && L.sm_type == AMGX_SM_JACOBI;
    if (jacobi && !L.Apre.empty()) {
      // one pass: r = b - A' b, x = omega * Dinv * b   (A' = A * omega*Dinv built at create time)
      product<1, EP_PRE>(L.Apre, b, r, EpArgs{b, nullptr, L.dinv.p, L.omega, x, ep_nt | (fold ? EPF_FOLD : 0)}, sp, true);
    } else if (sp.part == PART_INT) {
      return;                                  // the other forms are not split: they run completely in the boundary part
    } else if (jacobi && L.ncols > L.n && !fold) {
      // rank-partitioned level without a pre-smoothing image (block levels): x = omega * Dinv * b is needed on the ghost
      // rows too (their b and dinv entries came with the exchange / the setup), so it is formed in the gathered buffer
      diag_apply(L, b, L.tmp.p, false, L.ncols);
      residual_sm(L, L.tmp.p, b, r);
      copy(x, L.tmp.p, L.len());
    } else if (jacobi) {
      if (fold && L.bs > 1) {
        // x_pre = omega * Dinv * b into tmp; then ONE pass: r = b - A x_pre and z = x_pre + omega * Dinv * r
        diag_apply(L, b, L.tmp.p, false);
        product<1, EP_JAC>(L.A, L.tmp.p, x, EpArgs{b, L.tmp.p, L.dinv.p, L.omega, r, ep_nt}, Span(), true);
      } else {
        diag_apply(L, b, x, false);          // x = omega * Dinv * b      (x was zero, res == b)
        residual_sm(L, x, b, r);             // r = b - A x (the residual before the restriction: a pass of the level)
        if (fold) diag_apply(L, r, x, true); // z = x + omega * Dinv * r  (folded post-smoothing, see fold_prolongation)
      }
    } else if (P.plain && L.sm_type == AMGX_SM_CHEBY) {
      cheb_smooth(L, x, x, b, r, false, true, true);     // from zero: step 1 reads b, no SpMV
    } else if (P.plain && L.sm_type == AMGX_SM_GS) {
      // forward sweep from x = 0, then the residual by the identity the level's images allow
      sweep_from_zero(L, x, b, r);
      residual_after_zero(L, x, b, r);
    } else {
      zero(x, L.len());
      copy(r, b, L.len());
      struct FromZero { bool& f; explicit FromZero(bool& ff) : f(ff) { f = true; } ~FromZero() { f = false; } } scope(pre_from_zero);
      level_smooth(L, 0, x, b, r, true, true, true);
    }
  }

  // ------------------------------------------------------------------ the fused down launcher
  // The kernels' operands (b, dinv, omega, nt, x) in the three modes: what is gathered, what the epilogue combines it with, the
  // flags, and the x that only MODE 0 writes.  MODE 1 is launched without the nt flags.
  struct DownOps { const double *v, *d; double omega; int flags; double* xout; };
  DownOps down_ops_jacobi(const DevLevel& L, const double* b, double* x, bool fold) const { return {b, L.dinv.p, L.omega, ep_nt | (fold ? EPF_FOLD : 0), x}; }
  static DownOps down_ops_gsb(const DevLevel& L, const double* x) { return {x, L.gsb.cvec.p, 0.0, 0, nullptr}; }
  DownOps down_ops_cheb(const double* x, const double* b) const { return {x, b, 0.0, ep_nt, nullptr}; }

  // One fused down launch of level l as resolve_paths planned it (DownPlan, down_plan.hpp), then the sum of the partial sums into
  // b_coarse.  One branch per family; in it the value lists (down_plan.hpp) are dispatched once.  A list that does not hold the
  // plan's value cannot happen: make_down_plan asked the same list.
  // sp: interior part = the chunks of interior rows only; boundary part = the remaining chunks plus the sum, which needs all of them
  void down_launch(int l, const DownPlan& p, const DownOps& o, double* b_coarse, const Span sp = Span()) {
    const DevLevel& L = lev[l];
    if (!p.on) throw Err("fused down pass: the level has no plan for it");
    const DevRestrict& R = p.mode == 1 ? L.RG : L.RF;
    int64_t ca, cb;
    if (!down_chunk_range(p, sp, ca, cb)) throw Err("fused down pass: diagonal images and compact chunks are not split into interior / boundary parts");
    const int grid = (int)(cb - ca), c0 = (int)ca;
    const DevMatrix& M = down_image(L, p.mode, p.family == DOWN_FAM_LW);
    // (rank-partitioned level: the events go around the interior launch, which runs beside the halo exchange)
    const bool probe = probe_level == l && probe_kind == 8 && probe_e0 && sp.part != PART_BND;
    bool miss = false;                  // a value that its list does not hold
    auto pick = [&](auto list, int value, auto&& run) { if (!dispatch(list, value, run)) miss = true; };
    probed(probe, [&] {
      if (grid <= 0) return;
      if (p.family == DOWN_FAM_SELL) {
        pick(IntList<0, 1, 2>{}, p.mode, [&](auto MODE) {
          auto image = [&](auto view) {
            using V = std::remove_const_t<std::remove_pointer_t<decltype(view.val)>>;       // double / float
            // <rows per chunk, MODE, entries of P per thread, lanes per row, value type>
            auto sell = [&](auto FB, auto EPT, auto G) {
              launch(sell_pre_restrict_kernel<FB(), MODE(), EPT(), G(), V>, grid, FB(), 0, stream, M.n_rows, c0, M.n_slices, view, o.v, o.d, o.omega, o.flags,
                     o.xout, nullptr, R.chunk_slot.p, R.slot_ptr.p, R.w.p, R.fi.p, R.part.p, R.dest.p, R.slice_list.p);
            };
            // which (MODE, lanes) reaches which instantiation (pick sets `miss` where a list does not hold the value):
            //   MODE 0 / 2, lanes 2 / 4 / 8:  <512, MODE, 4, lanes>        (MODE 1 has no multi-lane form: a miss)
            //   MODE 0, one lane:             <256 / 512 / 1024, 0, 4 / 6, 1>
            //   MODE 1 / 2, one lane:         <512, MODE, 4 / 6, 1>
            if constexpr (MODE() != 1) { if (p.lanes > 1) return pick(DownSellLanes{}, p.lanes, [&](auto G) { sell(Int<DOWN_THREADS>{}, Int<DOWN_MULTI_EPT>{}, G); }); }
            if (p.lanes > 1) { miss = true; return; }
            if constexpr (MODE() == 0) pick(DownSizes{}, p.threads, [&](auto FB) { pick(DownEpt{}, p.ept, [&](auto EPT) { sell(FB, EPT, Int<1>{}); }); });
            else pick(DownEpt{}, p.ept, [&](auto EPT) { sell(Int<DOWN_THREADS>{}, EPT, Int<1>{}); });
          };
          // (MODE 2 is a smoother pass: the float kernel on the single-precision image where the level has one)
          // (... and MODE 0 on the float A' of a scalar Jacobi level; MODE 1 on the float `rest` of a scalar
          //  Gauss-Seidel level)
          if (p.f32) return image(M.sell.view32(M.val32.p));
          image(M.sell.view());
        });
      } else if (p.family == DOWN_FAM_WIN) {
        pick(IntList<0, 1>{}, p.mode, [&](auto MODE) { pick(DownEpt{}, p.ept, [&](auto EPT) {
          auto image = [&](auto view) {
            using V = std::remove_const_t<std::remove_pointer_t<decltype(view.val)>>;       // double / float
            launch(sell_win_pre_restrict_kernel<SELL_WIN, EPT(), MODE(), V>, grid, SELL_WIN, 0, stream, M.n_rows, c0, view, M.sell.rowloc.p, o.v, o.d, o.omega,
                   o.flags, o.xout, R.view());
          };
          if constexpr (MODE() == 1) { if (p.f32) return image(M.sell.view32(M.val32.p)); }
          image(M.sell.view());
        }); });
      } else if (p.family == DOWN_FAM_LW) {
        // long-row level: the local-window image (gathers from LDS), chunks of 512 / lanes rows
        const int32_t *cptr = p.mode == 1 ? L.gsb.lw_cptr.p : L.lw_cptr.p, *ccol = p.mode == 1 ? L.gsb.lw_ccol.p : L.lw_ccol.p;
        pick(IntList<0, 1>{}, p.mode, [&](auto MODE) { pick(DownLwLanes{}, p.lanes, [&](auto G) { pick(DownLwEpt{}, p.ept, [&](auto EPT) {
          auto image = [&](auto view) {
            using V = std::remove_const_t<std::remove_pointer_t<decltype(view.val)>>;       // double / float
            launch(sell_lw_pre_restrict_kernel<EPT(), G(), MODE(), V>, grid, DOWN_THREADS, 0, stream, M.n_rows, c0, M.n_slices, view, cptr, ccol, o.v, o.d,
                   o.omega, o.flags, o.xout, R.chunk_slot.p, R.slot_ptr.p, R.w.p, R.fi.p, R.part.p, R.dest.p);
          };
          if (p.f32) return image(M.sell.view32(M.val32.p));
          image(M.sell.view());
        }); }); });
      } else if (p.family == DOWN_FAM_DIA) {
        // symmetric diagonal image: 512-row chunks, one thread per row, whole level in one launch
        pick(DiaDiags{}, p.diags, [&](auto K) { pick(DownEpt{}, p.ept, [&](auto EPT) {
          auto image = [&](auto view) {
            using V = std::remove_const_t<std::remove_pointer_t<decltype(view.val)>>;       // double / float
            launch(dia_pre_restrict_kernel<K(), EPT(), V>, grid, DOWN_THREADS, 0, stream, (int)L.n, (int)((L.n + WAVE - 1) / WAVE), view, o.v, o.d, o.omega,
                   o.flags, o.xout, R.chunk_slot.p, R.slot_ptr.p, R.w.p, R.fi.p, R.part.p, R.dest.p, R.slice_list.p);
          };
          if (p.f32) image(L.dia.view32());
          else image(L.dia.view());
        }); });
      } else {
        // ... on box chunks: one 512-lane workgroup per box of grid lines
        pick(DiaBoxDiags{}, p.diags, [&](auto K) {
          auto image = [&](auto view) {
            using V = std::remove_const_t<std::remove_pointer_t<decltype(view.val)>>;       // double / float
            launch(dia_box_pre_restrict_kernel<K(), V>, grid, DOWN_THREADS, p.lds_bytes, stream, (int)L.n, view, R.box, R.box.box_rows(), o.v, o.d, o.omega,
                   o.flags, o.xout, R.chunk_slot.p, R.slot_ptr.p, R.w.p, R.fi.p, R.part.p, R.dest.p);
          };
          if (p.f32) image(L.dia.view32());
          else image(L.dia.view());
        });
      }
    });
    if (miss) throw Err("fused down pass: no kernel for the plan");
    if (!skip_rsum && sp.part != PART_INT) restrict_sum(l, R, b_coarse);
  }

  // down_launch on NV = 2 or 4 interleaved vectors (AMGX_MULTI_FUSE_DOWN): the same plan, the same operands (the
  // vectors of `o` interleaved; dinv of MODE 0 and c of MODE 1 per row), the whole level in one launch.  Which plans have a kernel is
  // down_nv_ok, for the diagonal-image families (AMGX_MULTI_FUSE_DOWN_DIA) down_nv_dia_ok and for the local-window family
  // (AMGX_MULTI_FUSE_DOWN_F32) down_nv_lw_ok (down_plan.hpp).  part_nv: n_slots * NV partial sums of the caller (the multi-vector work space), summed into b_coarse
  template <int NV>
  void down_launch_nv(int l, const DownPlan& p, const DownOps& o, double* part_nv, double* b_coarse) {
    const DevLevel& L = lev[l];
    if (!down_nv_ok(p, NV) && !down_nv_dia_ok(p, NV) && !down_nv_lw_ok(p, NV)) throw Err("fused multi-vector down pass: the level has no plan for it");
    const DevRestrict& R = p.mode == 1 ? L.RG : L.RF;
    const int grid = p.n_chunks;
    const DevMatrix& M = down_image(L, p.mode, p.family == DOWN_FAM_LW);
    bool miss = false;
    auto pick = [&](auto list, int value, auto&& run) { if (!dispatch(list, value, run)) miss = true; };
    if (grid > 0 && p.family == DOWN_FAM_DIA) {
      // symmetric diagonal image (AMGX_MULTI_FUSE_DOWN_DIA; the rule is down_nv_dia_ok): 512-row chunks
      pick(DiaDiags{}, p.diags, [&](auto K) { pick(DownEpt{}, p.ept, [&](auto EPT) {
        launch(dia_pre_restrict_nv_kernel<K(), EPT(), NV>, grid, DOWN_THREADS, 0, stream, (int)L.n, (int)((L.n + WAVE - 1) / WAVE), L.dia.view(), o.v, o.d, o.omega,
               o.flags, o.xout, R.chunk_slot.p, R.slot_ptr.p, R.w.p, R.fi.p, part_nv, R.dest.p, R.slice_list.p);
      }); });
    } else if (grid > 0 && p.family == DOWN_FAM_DIA_BOX) {
      // ... on box chunks; the dynamic LDS was allowed at create time where it exceeds 64 KB (dia_image, build_level.hpp)
      pick(DiaBoxDiags{}, p.diags, [&](auto K) {
        launch(dia_box_pre_restrict_nv_kernel<K(), NV>, grid, DOWN_THREADS, down_nv_dia_lds_bytes(p, NV), stream, (int)L.n, L.dia.view(), R.box, (int)p.box_rows,
               o.v, o.d, o.omega, o.flags, o.xout, R.chunk_slot.p, R.slot_ptr.p, R.w.p, R.fi.p, part_nv, R.dest.p);
      });
    } else if (grid > 0 && p.family == DOWN_FAM_SELL) {
      pick(IntList<0, 1, 2>{}, p.mode, [&](auto MODE) {
        auto image = [&](auto view) {
          using V = std::remove_const_t<std::remove_pointer_t<decltype(view.val)>>;       // double / float
          auto sell = [&](auto EPT, auto G) {
            launch(sell_pre_restrict_nv_kernel<DOWN_THREADS, MODE(), EPT(), G(), NV, V>, grid, DOWN_THREADS, 0, stream, M.n_rows, 0, M.n_slices, view, o.v, o.d,
                   o.omega, o.flags, o.xout, R.chunk_slot.p, R.slot_ptr.p, R.w.p, R.fi.p, part_nv, R.dest.p, R.slice_list.p);
          };
          if constexpr (MODE() != 1) { if (p.lanes > 1) return pick(DownSellLanes{}, p.lanes, [&](auto G) { sell(Int<DOWN_MULTI_EPT>{}, G); }); }
          if (p.lanes > 1) { miss = true; return; }
          pick(DownEpt{}, p.ept, [&](auto EPT) { sell(EPT, Int<1>{}); });
        };
        // (the float image as in down_launch: MODE 2 of a Chebyshev level, MODE 1 on `rest` of a scalar Gauss-Seidel level under
        //  AMGX_MULTI_FUSE_DOWN_F32; a float A' of MODE 0 never gets here: Multi::level_down refuses the level)
        if constexpr (MODE() != 0) { if (p.f32) return image(M.sell.view32(M.val32.p)); }
        image(M.sell.view());
      });
    } else if (grid > 0 && p.family == DOWN_FAM_LW) {
      // local-window image of `rest` (AMGX_MULTI_FUSE_DOWN_F32; the rule is down_nv_lw_ok): chunks of 512 / lanes rows;
      // the dynamic LDS was allowed at create time where it exceeds 64 KB (allow_down_nv_lw, build_level.hpp)
      pick(DownLwLanes{}, p.lanes, [&](auto G) { pick(DownLwEpt{}, p.ept, [&](auto EPT) {
        auto image = [&](auto view) {
          using V = std::remove_const_t<std::remove_pointer_t<decltype(view.val)>>;       // double / float
          launch(sell_lw_pre_restrict_nv_kernel<EPT(), G(), 1, NV, V>, grid, DOWN_THREADS, down_nv_lw_lds_bytes(p, NV), stream, M.n_rows, M.n_slices, view,
                 p.lw_max_list, L.gsb.lw_cptr.p, L.gsb.lw_ccol.p, o.v, o.d, R.chunk_slot.p, R.slot_ptr.p, R.w.p, R.fi.p, part_nv, R.dest.p);
        };
        if (p.f32) return image(M.sell.view32(M.val32.p));
        image(M.sell.view());
      }); });
    } else if (grid > 0) {
      RestrictMat rv = R.view();
      rv.part = part_nv;
      pick(DownEpt{}, p.ept, [&](auto EPT) {
        auto image = [&](auto view) {
          using V = std::remove_const_t<std::remove_pointer_t<decltype(view.val)>>;       // double / float
          launch(sell_win_pre_restrict_nv_kernel<SELL_WIN, EPT(), 1, NV, V>, grid, SELL_WIN, 0, stream, M.n_rows, 0, view, M.sell.rowloc.p, o.v, o.d, rv);
        };
        if (p.f32) return image(M.sell.view32(M.val32.p));
        image(M.sell.view());
      });
    }
    if (miss) throw Err("fused multi-vector down pass: no kernel for the plan");
    launch(restrict_sum_nv_kernel<NV>, grid_for((lev[l + 1].n + RSUM_R - 1) / RSUM_R * RSUM_G), BLOCK, 0, stream, lev[l + 1].n, R.optr.p, R.oidx.p, part_nv, b_coarse);
  }

  // pre-smoothing followed by the restriction of the residual (amg_matrix.cpp:193-212), fused where the level has a plan
  // sp: interior part = the row-parallel pass over the interior rows only; boundary part = the remaining rows plus
  // everything that needs all rows (partial-sum reduction / P^T gather)
  void pre_smooth_restrict(int l, double* x, const double* b, double* r, double* b_coarse, bool fold = false, const Span sp = Span()) {
    DevLevel& L = lev[l];
    if (fold && !L.paths.folded) throw Err("pre_smooth_restrict: level has no folded prolongation");
    const bool whole = sp.part == PART_ALL;     // (the residual forms run the whole level: a split level takes the unfused path)
    if (L.paths.jacobi_down()) down_launch(l, L.plan_rf, down_ops_jacobi(L, b, x, fold), b_coarse, sp);
    else if (L.paths.down == DOWN_CHEB && whole) {
      // Chebyshev pre-smoothing from zero, then residual on the SELL image of A + chunk-local restriction in one pass (r stays in LDS)
      cheb_smooth(L, x, x, b, r, false, false, true);
      down_launch(l, L.plan_rf, down_ops_cheb(x, b), b_coarse);
    } else if (L.paths.down == DOWN_GSB && whole) {
      // sweep from zero, then residual of the untouched part + chunk-local restriction in one pass (r stays in LDS)
      sweep_from_zero(L, x, b, r);
      residual_restrict_after_zero(l, x, b, r, b_coarse);
    } else {
      pre_smooth(L, x, b, r, fold, sp);
      if (sp.part != PART_INT) transfer_f2c(l, r, b_coarse);
    }
  }

  // residual_after_zero followed by the restriction b_coarse = P^T r; fused into one launch (r stays in LDS) where the level has
  // the plan for it
  void residual_restrict_after_zero(int l, const double* x, const double* b, double* r, double* b_coarse) {
    DevLevel& L = lev[l];
    if (L.paths.sweep == SWEEP_GSB && L.plan_rg.on) { down_launch(l, L.plan_rg, down_ops_gsb(L, x), b_coarse); return; }
    residual_after_zero(L, x, b, r);
    transfer_f2c(l, r, b_coarse);
  }

  // coarse-grid correction + post-smoothing: x += P x_c; SmoothBack(x, b, r, 0, 0, 0)   (amg_matrix.cpp:263-302)
  // fold: x holds z of the folded pre-smoothing pass; x' = z + Q x_c (see fold_prolongation)
  void post_smooth(int l, double* x, const double* b, double* r, const double* xc, bool fold = false, const Span sp = Span()) {
    DevLevel& L = lev[l];
    const LevelPaths& P = L.paths;
    const bool probe = probe_level == l && probe_kind == 9 && probe_e0;
    const bool probe_blk = probe_level == l && probe_kind == 11 && probe_e0;     // amgx_time_op op 11: the block sweep
    if (fold && !L.QLW.empty()) {
      // local-window form of Q: the coarse values a window needs are staged in LDS (sell_lw_win_spmv_kernel); interior / boundary
      // window ranges on rank-partitioned levels (the list of an interior window holds owned coarse columns only)
      const int64_t nw = (L.QLW.n_rows + SELL_WIN - 1) / SELL_WIN;
      int64_t wa, wb;
      unit_range(sp, SELL_WIN, nw, wa, wb);
      auto image = [&](auto view) {             // (the float image of a level with single-precision Jacobi images)
        using V = std::remove_const_t<std::remove_pointer_t<decltype(view.val)>>;
        launch(sell_lw_win_spmv_kernel<SELL_WIN, EP_AXPY, V>, (int)(wb - wa), SELL_WIN, 0, stream, L.QLW.n_rows, (int)wa, view, L.QLW.sell.rowloc.p,
               L.qlw_cptr.p, L.qlw_ccol.p, xc, x, EpArgs{nullptr, x, nullptr, 1.0, nullptr, ep_nt & EPF_HOIST});
      };
      if (wb > wa) {
        if (L.QLW.has32()) image(L.QLW.sell.view32(L.QLW.val32.p));
        else image(L.QLW.sell.view());
      }
    } else if (fold) {
      mult_add(L.Q, 1.0, xc, x, x, sp, true);
    } else if (sp.part == PART_INT) {
      return;                                  // literal forms are driven stage by stage (Dist), not through this function
    } else if (P.plain && L.sm_type == AMGX_SM_JACOBI) {
      mult_add(L.P, 1.0, xc, x, L.tmp.p);  // tmp = x + P x_c
      jacobi_fused(L, L.tmp.p, b, x);      // x = tmp + omega * Dinv * (b - A tmp); res is not needed afterwards
    } else if (P.plain && L.sm_type == AMGX_SM_CHEBY) {
      // k out-of-place passes follow: x + P x_c goes where the last of them lands in x
      double* t = cheb_place(cheb_passes(L.cheb_degree, ChebEntry::ITERATE), x, L.tmp.p);
      mult_add(L.P, 1.0, xc, x, t);
      cheb_smooth(L, t, x, b, r, false, false, false);
    } else if (P.plain && P.hybrid() && (P.sweep != SWEEP_GSB || L.n == L.ncols)) {
      double* const t = P.in_place ? x : L.tmp.p;
      mult_add(L.P, 1.0, xc, x, t);        // t = x + P x_c
      probed(probe || (probe_blk && P.bgsb()), [&] { sweep(L, 1, t, x, b); });      // backward sweep, t -> x: ONE launch, or one per block colour in place
    } else {
      add_c2f(l, 1.0, x, xc);
      probed(probe_blk && P.plain, [&] { level_smooth(L, 1, x, b, r, false, false, false); });    // (plain, no residual: the sweep alone)
    }
  }

  // ------------------------------------------------------------------ cycles
  // l0: first level of the (sub-)cycle; x, b are the vectors of that level (l0 > 0: build_dense_tail)
  void cycle_v(double* x, const double* b, int l0 = 0) {
    const int L = n_levels();
    if (dense_level >= 0 && dense_level == l0) {           // the whole (sub-)cycle is the dense operator: x = B b
      Range rg("rest");
      launch(dense_op_gemv_kernel, wave_grid(dense_n), BLOCK, 0, stream,
                         dense_n, dense_ld, dense_op.p, b, x);
      return;
    }
    if (l0 == L - 1) { coarse_solve(b, x); return; }
    const bool dense = dense_level > l0;
    const bool tail = !dense && tail_level > 0 && l0 == 0;
    const int T = dense ? dense_level : (tail ? tail_level : L - 1);     // levels >= T: one dense GEMV / tail_kernel
    for (int l = l0; l < T; ++l) {
      Range rg(level_range_name(l));
      double* xl = l == l0 ? x : lev[l].x.p;
      const double* bl = l == l0 ? b : lev[l].rhs.p;
      pre_smooth_restrict(l, xl, bl, lev[l].res.p, lev[l + 1].rhs.p, folded(lev[l]));
    }
    if (dense) {
      Range rg("rest");                                    // levels >= dense_level incl. "coarse inv": x_T = B b_T
      launch(dense_op_gemv_kernel, wave_grid(dense_n), BLOCK, 0, stream,
                         dense_n, dense_ld, dense_op.p, lev[T].rhs.p, lev[T].x.p);
    } else if (tail) {
      Range rg("rest");                                    // the coarse tail incl. "coarse inv" in one workgroup
      launch(tail_kernel, 1, TAIL_BLOCK, 0, stream, tail_ops, tail_prog.p);
    } else coarse_solve(lev[L - 1].rhs.p, lev[L - 1].x.p);
    for (int l = T - 1; l >= l0; --l) {
      Range rg(level_range_name(l));
      double* xl = l == l0 ? x : lev[l].x.p;
      const double* bl = l == l0 ? b : lev[l].rhs.p;
      post_smooth(l, xl, bl, lev[l].res.p, lev[l + 1].x.p, folded(lev[l]));
    }
  }

  // plain W-cycle (the reference additionally runs and discards a V-like pass at level 0, amg_matrix.cpp:46-64)
  void w_rec(int l, double* x0, const double* b0) {
    const int L = n_levels();
    if (l + 1 < L) {
      DevLevel& V = lev[l];
      double* xl = l == 0 ? x0 : V.x.p;
      const double* bl = l == 0 ? b0 : V.rhs.p;
      double* rl = V.res.p;
      pre_smooth_restrict(l, xl, bl, rl, lev[l + 1].rhs.p);
      w_rec(l + 1, x0, b0);
      add_c2f(l, 1.0, xl, lev[l + 1].x.p);
      level_smooth(V, 1, xl, bl, rl, false, true, false);
      level_smooth(V, 0, xl, bl, rl, true, true, false);
      transfer_f2c(l, rl, lev[l + 1].rhs.p);
      w_rec(l + 1, x0, b0);
      post_smooth(l, xl, bl, rl, lev[l + 1].x.p);
    } else {
      if (L == 1) coarse_solve(b0, x0);
      else coarse_solve(lev[L - 1].rhs.p, lev[L - 1].x.p);
    }
  }

  // AMGMatrix::SmoothVFromLevel, amg_matrix.cpp:310-374
  void smooth_v_from_level(int start, double* x, const double* b, double* res, bool ru, bool ur, bool xz) {
    const int L = n_levels();
    level_smooth(lev[start], 0, x, b, res, ru, true, xz);
    transfer_f2c(start, res, lev[start + 1].rhs.p);
    if (start + 2 < L)
      for (int l = start + 1; l + 1 < L; ++l) {
        pre_smooth_restrict(l, lev[l].x.p, lev[l].rhs.p, lev[l].res.p, lev[l + 1].rhs.p);
      }
    coarse_solve(lev[L - 1].rhs.p, lev[L - 1].x.p);
    if (start + 2 < L)
      for (int l = L - 2; l > start; --l) post_smooth(l, lev[l].x.p, lev[l].rhs.p, lev[l].res.p, lev[l + 1].x.p);
    add_c2f(start, 1.0, x, lev[start + 1].x.p);
    level_smooth(lev[start], 1, x, b, res, false, ur, false);
  }

  // AMGMatrix::SmoothBS, amg_matrix.cpp:110-157
  void cycle_bs(double* x, const double* b) {
    const int L = n_levels();
    if (L == 1) { coarse_solve(b, x); return; }
    for (int l = 0; l + 1 < L; ++l) {
      double* xl = l == 0 ? x : lev[l].x.p;
      const double* bl = l == 0 ? b : lev[l].rhs.p;
      double* rl = lev[l].res.p;
      zero(xl, lev[l].len());
      copy(rl, bl, lev[l].len());
      smooth_v_from_level(l, xl, bl, rl, true, true, true);
      transfer_f2c(l, rl, lev[l + 1].rhs.p);
    }
    coarse_solve(lev[L - 1].rhs.p, lev[L - 1].x.p);
    for (int l = L - 2; l >= 0; --l) {
      double* xl = l == 0 ? x : lev[l].x.p;
      const double* bl = l == 0 ? b : lev[l].rhs.p;
      add_c2f(l, 1.0, xl, lev[l + 1].x.p);
      smooth_v_from_level(l, xl, bl, lev[l].res.p, false, false, false);
    }
  }

  void do_cycle(double* x, const double* b) {
    Range rg("AMGMatrix::Mult");
    if (cycle == AMGX_CYCLE_W) w_rec(0, x, b);
    else if (cycle == AMGX_CYCLE_BS) cycle_bs(x, b);
    else cycle_v(x, b);
  }

  // one application, optionally through a captured graph keyed by the vector addresses
  void run_cycle(double* x, const double* b, bool graph_ok) {
    // the legacy default stream cannot be captured: launch directly there
    if (!(use_graph && graph_ok) || stream == nullptr) { do_cycle(x, b); return; }
    graphs.run(GraphKey{b, x, 0}, stream, [&] { do_cycle(x, b); });
  }

  void drop_graphs() {
    graphs.drop();
    if (multi) multi_drop_graphs(multi);
  }
};

// ---------------------------------------------------------------------------------------------------
// construction
// ---------------------------------------------------------------------------------------------------

struct HostCsr {
  std::vector<int64_t> rowptr;
  std::vector<int32_t> col;
  std::vector<double> val;
};
static void use_csr(amgx_matrix& M, const HostCsr& c) { M.rowptr = c.rowptr.data(); M.col = c.col.data(); M.val = c.val.data(); }

}  // namespace amgx
#include "devbuild.hpp"
#include "gs_images.hpp"        // build_gs, build_gsb, build_bgsb and their AMGX_VERIFY_IMAGES cross-checks
#include "spgemm.hpp"
namespace amgx {

// ---------------------------------------------------------------------------------------------------
// Folded post-smoothing.  In the V(1,1) Jacobi cycle the post-smoothing step (amg_matrix.cpp:263-302)
//     x' = t + omega*Dinv*(b - A t),   t = x + P x_c
// is affine in (x, x_c):  x' = [x + omega*Dinv*(b - A x)] + (I - omega*Dinv*A) P x_c = z + Q x_c,  where b - A x is the
// residual the pre-smoothing pass already has in registers.  So the pre-smoothing kernel writes z instead of x (EPF_FOLD)
// and the whole post-smoothing is ONE SpMV-AXPY with Q = (I - omega*Dinv*A) P, built once here (host, threads over row
// ranges).  Q has about half the entries of A (cfg 2: 7.8 vs 14.8 per row), and the pass over P and the round trip of
// t through HBM disappear.  Same result up to rounding; AMGX_NO_FOLD=1 runs the literal sequence.
// (block form: A has bs x bs blocks, P and Q bs x bc blocks, dinv bs x bs per block row)
static void fold_prolongation(const amgx_matrix& A, const amgx_matrix& P, const double* dinv, double omega, HostCsr& Q) {
  const int64_t n = A.n_rows, nc = P.n_cols;
  const int bs = A.br, bc = P.bc, bb = bs * bc;
  int T = (int)std::min<int64_t>(std::max(1u, std::thread::hardware_concurrency()), 32);
  if (const char* e = std::getenv("OMP_NUM_THREADS")) T = std::max(1, std::min(T, std::atoi(e)));
  T = (int)std::max<int64_t>(1, std::min<int64_t>(T, n / 4096 + 1));
  struct Part { std::vector<int32_t> col; std::vector<double> val; };
  std::vector<Part> parts(T);
  Q.rowptr.assign(n + 1, 0);
  auto work = [&](int t) {
    const int64_t r0 = n * t / T, r1 = n * (t + 1) / T;
    std::vector<int32_t> mark(nc, -1), cols, order;
    std::vector<double> own, acc, tmp(bb);    // own = P_i blocks, acc = sum_j A_ij P_j blocks (same slot numbering)
    Part& out = parts[t];
    for (int64_t i = r0; i < r1; ++i) {
      cols.clear(); own.clear(); acc.clear();
      auto slot = [&](int32_t c) -> int32_t {
        int32_t& m = mark[c];
        if (m < 0) { m = (int32_t)cols.size(); cols.push_back(c); own.resize(own.size() + bb, 0.0); acc.resize(acc.size() + bb, 0.0); }
        return m;
      };
      for (int64_t k = P.rowptr[i]; k < P.rowptr[i + 1]; ++k) {
        const int32_t sl = slot(P.col[k]);          // (may reallocate own: take the pointer afterwards)
        double* o = own.data() + (size_t)sl * bb;
        for (int e = 0; e < bb; ++e) o[e] += P.val[k * bb + e];
      }
      const double* d = dinv + i * bs * bs;
      bool dzero = true;
      for (int e = 0; e < bs * bs; ++e) if (d[e] != 0.0) { dzero = false; break; }
      if (!dzero)
        for (int64_t k = A.rowptr[i]; k < A.rowptr[i + 1]; ++k) {
          const int64_t j = A.col[k];
          if (j >= P.n_rows) continue;
          const double* a = A.val + k * bs * bs;
          for (int64_t q = P.rowptr[j]; q < P.rowptr[j + 1]; ++q) {
            const double* pv = P.val + q * bb;
            const int32_t sl = slot(P.col[q]);       // (may reallocate acc: take the pointer afterwards)
            double* o = acc.data() + (size_t)sl * bb;
            for (int r = 0; r < bs; ++r)
              for (int m = 0; m < bs; ++m) {
                const double arm = a[r * bs + m];
                for (int c = 0; c < bc; ++c) o[r * bc + c] += arm * pv[m * bc + c];
              }
          }
        }
      order.resize(cols.size());
      for (size_t q = 0; q < cols.size(); ++q) order[q] = (int32_t)q;
      std::sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return cols[a] < cols[b]; });
      for (int32_t q : order) {
        const double* o = own.data() + (size_t)q * bb;
        const double* sa = acc.data() + (size_t)q * bb;
        // Q block = P block - omega * Dinv_i * (A P) block
        for (int r = 0; r < bs; ++r)
          for (int c = 0; c < bc; ++c) {
            double u = 0.0;
            for (int m = 0; m < bs; ++m) u += d[r * bs + m] * sa[m * bc + c];
            tmp[r * bc + c] = o[r * bc + c] - omega * u;
          }
        out.col.push_back(cols[q]);
        out.val.insert(out.val.end(), tmp.begin(), tmp.end());
        mark[cols[q]] = -1;
      }
      Q.rowptr[i + 1] = (int64_t)cols.size();
    }
  };
  if (T == 1) work(0);
  else {
    std::vector<std::thread> th;
    for (int t = 0; t < T; ++t) th.emplace_back(work, t);
    for (auto& x : th) x.join();
  }
  for (int64_t i = 0; i < n; ++i) Q.rowptr[i + 1] += Q.rowptr[i];
  Q.col.resize((size_t)Q.rowptr[n]);
  Q.val.resize((size_t)Q.rowptr[n] * bb);
  for (int t = 0; t < T; ++t) {
    const int64_t o = Q.rowptr[n * t / T];
    std::copy(parts[t].col.begin(), parts[t].col.end(), Q.col.begin() + o);
    std::copy(parts[t].val.begin(), parts[t].val.end(), Q.val.begin() + o * bb);
    Part().col.swap(parts[t].col); Part().val.swap(parts[t].val);
  }
}

// ---------------------------------------------------------------------------------------------------
// Colour-major numbering of Gauss-Seidel levels.  A colour kernel touches the rows of ONE colour; in the caller's
// numbering those are every ~8th row, so x, b and dinv were read and written with 1/8 line utilisation, eight times
// per sweep (GS V-cycle at cfg 2: colour kernels at 2-3 TB/s).  With the rows of a colour stored contiguously the
// same kernels stream.  The renumbering is internal: the host matrices are permuted once here (P A P^T, rows of P,
// columns of P^T, ...) and the entry points translate vectors at the boundary (two extra passes over b and x per
// application, ~60 us at cfg 2, against ~400 us saved).  AMGX_NO_GS_PERM=1 keeps the caller's numbering.
struct LevelPerm {
  std::vector<int32_t> perm, iperm;       // perm[new] = old, iperm[old] = new; empty = identity
  HostCsr A, P, PT;
  std::vector<double> dinv;
  std::vector<uint8_t> free_dofs;
  std::vector<int32_t> color;
};

// rows reordered by rperm (new -> old, or null), columns renumbered by ciperm (old -> new, or null), rows re-sorted
static void permute_matrix(const amgx_matrix& M, const int32_t* rperm, const int32_t* ciperm, HostCsr& out) {
  const int64_t n = M.n_rows;
  const int bb = M.br * M.bc;
  out.rowptr.assign(n + 1, 0);
  for (int64_t i = 0; i < n; ++i) { const int64_t o = rperm ? rperm[i] : i; out.rowptr[i + 1] = out.rowptr[i] + (M.rowptr[o + 1] - M.rowptr[o]); }
  const int64_t nnz = out.rowptr[n];
  out.col.resize((size_t)nnz);
  out.val.resize((size_t)nnz * bb);
  int T = (int)std::min<int64_t>(std::max(1u, std::thread::hardware_concurrency()), 16);
  if (const char* e = std::getenv("OMP_NUM_THREADS")) T = std::max(1, std::min(T, std::atoi(e)));
  T = (int)std::max<int64_t>(1, std::min<int64_t>(T, n / 8192 + 1));
  auto work = [&](int t) {
    std::vector<std::pair<int32_t, int64_t>> row;
    for (int64_t i = n * t / T; i < n * (t + 1) / T; ++i) {
      const int64_t o = rperm ? rperm[i] : i;
      row.clear();
      for (int64_t k = M.rowptr[o]; k < M.rowptr[o + 1]; ++k) row.emplace_back(ciperm ? ciperm[M.col[k]] : M.col[k], k);
      if (ciperm) std::sort(row.begin(), row.end());
      int64_t w = out.rowptr[i];
      for (const auto& e : row) {
        out.col[w] = e.first;
        std::copy(M.val + e.second * bb, M.val + (e.second + 1) * bb, out.val.begin() + w * bb);
        ++w;
      }
    }
  };
  if (T == 1) work(0);
  else {
    std::vector<std::thread> th;
    for (int t = 0; t < T; ++t) th.emplace_back(work, t);
    for (auto& x : th) x.join();
  }
}


// fills pl (mutable copies of the level descriptors) with colour-major versions of the GS levels; store owns the data
static void permute_gs_levels(const Knobs& K, const amgx_hierarchy_desc* d, std::vector<amgx_level_desc>& pl, std::vector<LevelPerm>& store) {
  const int L = d->n_levels;
  // Measured NON-win (profiles/r01/gs_perm.txt): the colour kernels gain 7-20 %, but the transfers lose far more
  // (P^T gathers its ~30 fine residuals per coarse row from 8 colour blocks: 129 -> 370 us; P: 78 -> 132 us) and the two
  // translation passes cost 125 us: cycle 2.35 -> 2.54 ms at cfg 2.  Off unless AMGX_GS_PERM=1 (kept under test).
  if (!K.gs_perm) return;
  for (int l = 0; l < L; ++l) if (pl[l].A.n_rows != pl[l].A.n_cols) return;     // rank-partitioned handle: vectors carry ghosts
  bool any = false;
  for (int l = 0; l + 1 < L; ++l) {
    const amgx_level_desc& s = pl[l];
    if (s.sm_type != AMGX_SM_GS || !s.color || s.n_colors <= 0 || s.A.n_rows < 2) continue;
    const int64_t n = s.A.n_rows;
    LevelPerm& lp = store[l];
    // stable counting sort by colour, rows without a colour (non-free) last
    std::vector<int64_t> start(s.n_colors + 2, 0);
    for (int64_t i = 0; i < n; ++i) { const int c = s.color[i]; if (c >= s.n_colors) throw Err("colour index out of range"); start[(c < 0 ? s.n_colors : c) + 1]++; }
    for (int c = 0; c <= s.n_colors; ++c) start[c + 1] += start[c];
    lp.perm.resize(n); lp.iperm.resize(n);
    for (int64_t i = 0; i < n; ++i) { const int c = s.color[i] < 0 ? s.n_colors : s.color[i]; const int64_t q = start[c]++; lp.perm[q] = (int32_t)i; lp.iperm[i] = (int32_t)q; }
    any = true;
  }
  if (!any) return;
  for (int l = 0; l < L; ++l) {
    amgx_level_desc& s = pl[l];
    LevelPerm& lp = store[l];
    const bool me = !lp.perm.empty();
    const bool nxt = l + 1 < L && !store[l + 1].perm.empty();
    if (me) {
      const int64_t n = s.A.n_rows;
      const int b2 = s.A.br * s.A.br;
      permute_matrix(s.A, lp.perm.data(), lp.iperm.data(), lp.A);
      use_csr(s.A, lp.A);
      if (s.dinv) { lp.dinv.resize((size_t)n * b2); for (int64_t i = 0; i < n; ++i) std::copy(s.dinv + (int64_t)lp.perm[i] * b2, s.dinv + ((int64_t)lp.perm[i] + 1) * b2, lp.dinv.begin() + i * b2); s.dinv = lp.dinv.data(); }
      if (s.free_dofs) { lp.free_dofs.resize(n); for (int64_t i = 0; i < n; ++i) lp.free_dofs[i] = s.free_dofs[lp.perm[i]]; s.free_dofs = lp.free_dofs.data(); }
      if (s.color) { lp.color.resize(n); for (int64_t i = 0; i < n; ++i) lp.color[i] = s.color[lp.perm[i]]; s.color = lp.color.data(); }
    }
    if ((me || nxt) && l + 1 < L && s.P.rowptr) {
      permute_matrix(s.P, me ? lp.perm.data() : nullptr, nxt ? store[l + 1].iperm.data() : nullptr, lp.P);
      use_csr(s.P, lp.P);
      permute_matrix(s.PT, nxt ? store[l + 1].perm.data() : nullptr, me ? lp.iperm.data() : nullptr, lp.PT);
      use_csr(s.PT, lp.PT);
    }
  }
}

}  // namespace amgx
#include "dense_spd.hpp"
#include "build_level.hpp"

// ---------------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------------

struct amgx_handle_t { amgx::Handle* h; };

namespace {
thread_local std::string g_create_err;

template <class F>
int guard(amgx_handle hh, F&& f) {
  try {
    if (!hh || !hh->h) throw amgx::Err("null handle");
    HIPCHK(hipSetDevice(hh->h->device));
    f(*hh->h);
    return 0;
  } catch (const std::exception& e) {
    if (hh && hh->h) hh->h->err = e.what(); else g_create_err = e.what();
    return 1;
  }
}

// stage host vectors on the device when the caller passed host pointers
struct Staged {
  amgx::Handle& h;
  bool host;
  Staged(amgx::Handle& hh, int flags) : h(hh), host(!(flags & AMGX_DEVICE_PTR)) {}
  static void fit(amgx::DevBuf<double>& b, int64_t n) { if ((int64_t)b.n < n) b.alloc(n); }
  // lvl >= 0: the vector belongs to that level; if the level is stored in colour-major numbering the device copy is
  // renumbered (device pointers too: the work then runs on the staging buffers)
  const double* in(int slot, const double* p, int64_t n, int lvl = -1) {
    if (!p) return p;
    const bool pm = h.permuted(lvl);
    if (!host && !pm) return p;
    const double* src = p;
    if (host) {
      amgx::DevBuf<double>& dst = pm ? h.stage_raw[slot] : h.stage[slot];
      fit(dst, n);
      HIPCHK(hipMemcpyAsync(dst.p, p, n * sizeof(double), hipMemcpyHostToDevice, h.stream));
      if (!pm) return dst.p;
      src = dst.p;
    }
    fit(h.stage[slot], n);
    h.perm_gather(lvl, src, h.stage[slot].p);
    return h.stage[slot].p;
  }
  double* inout(int slot, double* p, int64_t n, bool load, int lvl = -1) {
    if (!p) return p;
    const bool pm = h.permuted(lvl);
    if (!host && !pm) return p;
    if (load) return const_cast<double*>(in(slot, p, n, lvl));
    fit(h.stage[slot], n);
    return h.stage[slot].p;
  }
  void out(int slot, double* p, int64_t n, int lvl = -1) {
    if (!p) return;
    const bool pm = h.permuted(lvl);
    if (!host && !pm) return;
    const double* src = h.stage[slot].p;
    if (pm) {
      double* dst = p;
      if (host) { fit(h.stage_raw[slot], n); dst = h.stage_raw[slot].p; }
      h.perm_scatter(lvl, src, dst);
      src = dst;
    }
    if (host) HIPCHK(hipMemcpyAsync(p, src, n * sizeof(double), hipMemcpyDeviceToHost, h.stream));
  }
  void finish() { if (host) HIPCHK(hipStreamSynchronize(h.stream)); }
};
}  // namespace

extern "C" {

const char* amgx_last_error(amgx_handle h) { return (h && h->h) ? h->h->err.c_str() : g_create_err.c_str(); }

int amgx_create(const amgx_hierarchy_desc* desc, amgx_handle* out) {
  try {
    if (!out) throw amgx::Err("amgx_create: null output");
    amgx::Handle* h = amgx::create(desc, amgx::Knobs::from_env());
    *out = new amgx_handle_t{h};
    return 0;
  } catch (const std::exception& e) { g_create_err = e.what(); return 1; }
}

int amgx_destroy(amgx_handle h) {
  if (!h) return 0;
  if (h->h) { (void)hipSetDevice(h->h->device); (void)hipDeviceSynchronize(); delete h->h; }
  delete h;
  return 0;
}

int amgx_device_count(int32_t* n) {
  if (!n) return 1;
  int nd = 0;
  *n = (hipGetDeviceCount(&nd) == hipSuccess) ? nd : 0;
  return 0;
}

// ---- setup products on the device (spgemm.hpp) -------------------------------------------------------
int amgx_spgemm(const amgx_matrix* A, const amgx_matrix* B, amgx_csr_result* out, int64_t* n_rows, int64_t* nnz) {
  try {
    if (!A || !B || !out) throw amgx::Err("amgx_spgemm: null argument");
    *out = nullptr;
    if (A->n_cols != B->n_rows || A->bc != B->br) throw amgx::Err("amgx_spgemm: dimension mismatch");
    if (A->br * B->bc > 36 || A->br < 1 || A->bc < 1 || B->bc < 1) return 2;
    amgx::SpCsr a, b;
    a.upload(*A);
    b.upload(*B);
    auto r = std::make_unique<amgx::SpCsr>();
    if (!amgx::dev_spgemm(a, b, *r)) return 2;
    if (n_rows) *n_rows = r->n_rows;
    if (nnz) *nnz = r->nnz;
    *out = reinterpret_cast<amgx_csr_result>(r.release());
    return 0;
  } catch (const std::exception& e) { g_create_err = e.what(); return 1; }
}

int amgx_galerkin(const amgx_matrix* PT, const amgx_matrix* A, const amgx_matrix* P, amgx_csr_result* out, int64_t* n_rows, int64_t* nnz) {
  try {
    if (!PT || !A || !P || !out) throw amgx::Err("amgx_galerkin: null argument");
    *out = nullptr;
    if (PT->n_cols != A->n_rows || A->n_cols != P->n_rows || PT->bc != A->br || A->bc != P->br) throw amgx::Err("amgx_galerkin: dimension mismatch");
    for (const amgx_matrix* m : {PT, A, P}) if (m->br < 1 || m->bc < 1 || m->br * m->bc > 36) return 2;
    if (PT->br * P->bc > 36) return 2;
    amgx::SpCsr pta;
    {
      amgx::SpCsr pt, a;
      pt.upload(*PT);
      a.upload(*A);
      if (!amgx::dev_spgemm(pt, a, pta)) return 2;
    }
    amgx::SpCsr p;
    p.upload(*P);
    auto r = std::make_unique<amgx::SpCsr>();
    if (!amgx::dev_spgemm(pta, p, *r)) return 2;
    if (n_rows) *n_rows = r->n_rows;
    if (nnz) *nnz = r->nnz;
    *out = reinterpret_cast<amgx_csr_result>(r.release());
    return 0;
  } catch (const std::exception& e) { g_create_err = e.what(); return 1; }
}

int amgx_csr_result_fetch(amgx_csr_result res, int64_t* rowptr, int32_t* col, double* val) {
  std::unique_ptr<amgx::SpCsr> r(reinterpret_cast<amgx::SpCsr*>(res));
  try {
    if (!r) throw amgx::Err("amgx_csr_result_fetch: null result");
    if (rowptr) HIPCHK(hipMemcpy(rowptr, r->rowptr.p, (size_t)(r->n_rows + 1) * sizeof(int64_t), hipMemcpyDeviceToHost));
    if (col && r->nnz) HIPCHK(hipMemcpy(col, r->col.p, (size_t)r->nnz * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (val && r->nnz) HIPCHK(hipMemcpy(val, r->val.p, (size_t)r->nnz * r->br * r->bc * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
  } catch (const std::exception& e) { g_create_err = e.what(); return 1; }
}

int amgx_set_stream(amgx_handle hh, void* s) {
  return guard(hh, [&](amgx::Handle& h) {
    hipStream_t ns = (hipStream_t)s;     // NULL = the legacy default stream (what torch uses unless told otherwise)
    if (ns != h.stream) { HIPCHK(hipStreamSynchronize(h.stream)); h.drop_graphs(); h.stream = ns; }
  });
}

int amgx_synchronize(amgx_handle hh) { return guard(hh, [&](amgx::Handle& h) { HIPCHK(hipStreamSynchronize(h.stream)); }); }

int amgx_apply(amgx_handle hh, const double* b, double* x, int b_status, int flags) {
  (void)b_status;   // single GPU: DISTRIBUTED == CUMULATED (b.Distribute() is a no-op, amg_matrix.cpp:164)
  return guard(hh, [&](amgx::Handle& h) {
    if (!b || !x) throw amgx::Err("amgx_apply: null vector");
    if (b == x) throw amgx::Err("amgx_apply: b and x must not alias");
    const int64_t n = h.lev[0].len();
    Staged st(h, flags);
    const double* db = st.in(0, b, n, 0);
    double* dx = st.inout(1, x, n, false, 0);
    h.run_cycle(dx, db, !(flags & AMGX_NO_GRAPH));
    st.out(1, x, n, 0);
    st.finish();
  });
}

int amgx_apply_add(amgx_handle hh, double s, const double* b, double* x, int flags) {
  return guard(hh, [&](amgx::Handle& h) {
    if (!b || !x) throw amgx::Err("amgx_apply_add: null vector");
    const int64_t n = h.lev[0].len();
    Staged st(h, flags);
    const double* db = st.in(0, b, n, 0);
    double* dx = st.inout(1, x, n, true, 0);
    h.run_cycle(h.lev[0].x.p, db, !(flags & AMGX_NO_GRAPH));     // cycle into x_level[0] (amg_matrix.cpp:385-389)
    h.axpy(n, s, h.lev[0].x.p, dx);
    st.out(1, x, n, 0);
    st.finish();
  });
}

int amgx_smooth(amgx_handle hh, int level, int dir, double* x, const double* b, double* res,
                int res_updated, int update_res, int x_zero, int flags) {
  return guard(hh, [&](amgx::Handle& h) {
    if (level < 0 || level >= h.n_levels()) throw amgx::Err("amgx_smooth: level out of range");
    amgx::DevLevel& L = h.lev[level];
    if (!L.dinv.p) throw amgx::Err("amgx_smooth: level has no smoother");
    if (!x || !b || !res) throw amgx::Err("amgx_smooth: null vector");
    const int64_t n = L.len();
    Staged st(h, flags);
    double* dx = st.inout(0, x, L.ext_len(), true, level);        // ghost entries (if any) are read, never written
    const double* db = st.in(1, b, n, level);
    double* dr = st.inout(2, res, n, true, level);
    h.level_smooth(L, dir, dx, db, dr, res_updated != 0, update_res != 0, x_zero != 0);
    st.out(0, x, n, level);
    st.out(2, res, n, level);
    st.finish();
  });
}

int amgx_smooth_v_from_level(amgx_handle hh, int level, double* x, const double* b, double* res,
                             int res_updated, int update_res, int x_zero, int flags) {
  return guard(hh, [&](amgx::Handle& h) {
    if (level < 0 || level + 1 >= h.n_levels()) throw amgx::Err("amgx_smooth_v_from_level: level out of range");
    const int64_t n = h.lev[level].len();
    Staged st(h, flags);
    double* dx = st.inout(0, x, n, true, level);
    const double* db = st.in(1, b, n, level);
    double* dr = st.inout(2, res, n, true, level);
    h.smooth_v_from_level(level, dx, db, dr, res_updated != 0, update_res != 0, x_zero != 0);
    st.out(0, x, n, level);
    st.out(2, res, n, level);
    st.finish();
  });
}

int amgx_residual(amgx_handle hh, int level, const double* x, const double* b, double* r, int flags) {
  return guard(hh, [&](amgx::Handle& h) {
    if (level < 0 || level >= h.n_levels()) throw amgx::Err("amgx_residual: level out of range");
    if (!x || !b || !r || x == r) throw amgx::Err("amgx_residual: bad vectors");
    amgx::DevLevel& L = h.lev[level];
    Staged st(h, flags);
    const double* dx = st.in(0, x, L.ext_len(), level);
    const double* db = st.in(1, b, L.len(), level);
    double* dr = st.inout(2, r, L.len(), false, level);
    h.residual(L.A, dx, db, dr);
    st.out(2, r, L.len(), level);
    st.finish();
  });
}

int amgx_jacobi_pre(amgx_handle hh, int level, const double* b, double* x, double* r, int flags) {
  return guard(hh, [&](amgx::Handle& h) {
    if (level < 0 || level >= h.n_levels()) throw amgx::Err("amgx_jacobi_pre: level out of range");
    amgx::DevLevel& L = h.lev[level];
    if (!L.dinv.p || L.sm_type != AMGX_SM_JACOBI) throw amgx::Err("amgx_jacobi_pre: level has no Jacobi smoother");
    if (!b || !x || !r) throw amgx::Err("amgx_jacobi_pre: null vector");
    Staged st(h, flags);
    const double* db = st.in(0, b, L.ext_len(), level);
    double* dx = st.inout(1, x, L.len(), false, level);
    double* dr = st.inout(2, r, L.len(), false, level);
    h.pre_smooth(L, dx, db, dr);
    st.out(1, x, L.len(), level);
    st.out(2, r, L.len(), level);
    st.finish();
  });
}

int amgx_cycle_down(amgx_handle hh, int level, const double* b, double* x, double* b_coarse, int flags) {
  return guard(hh, [&](amgx::Handle& h) {
    if (level < 0 || level + 1 >= h.n_levels()) throw amgx::Err("amgx_cycle_down: level out of range");
    amgx::DevLevel& L = h.lev[level];
    if (!h.folded(L)) throw amgx::Err("amgx_cycle_down: level has no folded prolongation Q (use amgx_jacobi_pre / amgx_transfer_f2c)");
    if (!b || !x || !b_coarse) throw amgx::Err("amgx_cycle_down: null vector");
    Staged st(h, flags);
    const double* db = st.in(0, b, L.ext_len(), level);
    double* dx = st.inout(1, x, L.len(), false, level);
    double* dc = st.inout(2, b_coarse, h.lev[level + 1].len(), false, level + 1);
    h.pre_smooth_restrict(level, dx, db, L.res.p, dc, true);
    st.out(1, x, L.len(), level);
    st.out(2, b_coarse, h.lev[level + 1].len(), level + 1);
    st.finish();
  });
}

int amgx_cycle_up(amgx_handle hh, int level, double* x, const double* x_coarse, int flags) {
  return guard(hh, [&](amgx::Handle& h) {
    if (level < 0 || level + 1 >= h.n_levels()) throw amgx::Err("amgx_cycle_up: level out of range");
    amgx::DevLevel& L = h.lev[level];
    if (!h.folded(L)) throw amgx::Err("amgx_cycle_up: level has no folded prolongation Q (use amgx_prolong / amgx_jacobi_post)");
    if (!x || !x_coarse) throw amgx::Err("amgx_cycle_up: null vector");
    Staged st(h, flags);
    double* dx = st.inout(0, x, L.len(), true, level);
    const double* dc = st.in(1, x_coarse, L.Q.n_cols, level + 1);
    h.post_smooth(level, dx, nullptr, L.res.p, dc, true);
    st.out(0, x, L.len(), level);
    st.finish();
  });
}

int amgx_jacobi_post(amgx_handle hh, int level, const double* xin, const double* b, double* xout, int flags) {
  return guard(hh, [&](amgx::Handle& h) {
    if (level < 0 || level >= h.n_levels()) throw amgx::Err("amgx_jacobi_post: level out of range");
    amgx::DevLevel& L = h.lev[level];
    if (!L.dinv.p || L.sm_type != AMGX_SM_JACOBI) throw amgx::Err("amgx_jacobi_post: level has no Jacobi smoother");
    if (!xin || !b || !xout || xin == xout) throw amgx::Err("amgx_jacobi_post: bad vectors");
    Staged st(h, flags);
    const double* dxi = st.in(0, xin, L.ext_len(), level);
    const double* db = st.in(1, b, L.len(), level);
    double* dxo = st.inout(2, xout, L.len(), false, level);
    h.jacobi_fused(L, dxi, db, dxo);
    st.out(2, xout, L.len(), level);
    st.finish();
  });
}

int amgx_prolong(amgx_handle hh, int level, double fac, const double* x_in, const double* x_coarse, double* x_out, int flags) {
  return guard(hh, [&](amgx::Handle& h) {
    if (level < 0 || level + 1 >= h.n_levels()) throw amgx::Err("amgx_prolong: level out of range");
    if (!x_in || !x_coarse || !x_out) throw amgx::Err("amgx_prolong: null vector");
    Staged st(h, flags);
    const double* di = st.in(0, x_in, h.lev[level].len(), level);
    const double* dc = st.in(1, x_coarse, h.lev[level].P.n_cols * h.lev[level].P.bc, level + 1);
    double* dout = st.inout(2, x_out, h.lev[level].len(), false, level);
    h.mult_add(h.lev[level].P, fac, dc, di, dout);
    st.out(2, x_out, h.lev[level].len(), level);
    st.finish();
  });
}

int amgx_matvec(amgx_handle hh, int level, const double* x, double* y, int flags) {
  return guard(hh, [&](amgx::Handle& h) {
    if (level < 0 || level >= h.n_levels()) throw amgx::Err("amgx_matvec: level out of range");
    if (!x || !y || x == y) throw amgx::Err("amgx_matvec: bad vectors");
    const int64_t n = h.lev[level].len();
    Staged st(h, flags);
    const double* dx = st.in(0, x, h.lev[level].ext_len(), level);
    double* dy = st.inout(1, y, n, false, level);
    h.mult(h.lev[level].A, dx, dy);
    st.out(1, y, n, level);
    st.finish();
  });
}

int amgx_transfer_f2c(amgx_handle hh, int level, const double* xf, double* xc, int flags) {
  return guard(hh, [&](amgx::Handle& h) {
    if (level < 0 || level + 1 >= h.n_levels()) throw amgx::Err("amgx_transfer_f2c: level out of range");
    Staged st(h, flags);
    const double* df = st.in(0, xf, h.lev[level].len(), level);
    double* dc = st.inout(1, xc, h.lev[level + 1].len(), false, level + 1);
    h.transfer_f2c(level, df, dc);
    st.out(1, xc, h.lev[level + 1].len(), level + 1);
    st.finish();
  });
}

int amgx_add_c2f(amgx_handle hh, int level, double fac, double* xf, const double* xc, int flags) {
  return guard(hh, [&](amgx::Handle& h) {
    if (level < 0 || level + 1 >= h.n_levels()) throw amgx::Err("amgx_add_c2f: level out of range");
    Staged st(h, flags);
    double* df = st.inout(0, xf, h.lev[level].len(), true, level);
    const double* dc = st.in(1, xc, h.lev[level + 1].len(), level + 1);
    h.add_c2f(level, fac, df, dc);
    st.out(0, xf, h.lev[level].len(), level);
    st.finish();
  });
}

int amgx_coarse_solve(amgx_handle hh, const double* rhs, double* x, int flags) {
  return guard(hh, [&](amgx::Handle& h) {
    const int64_t n = h.lev.back().len();
    Staged st(h, flags);
    const double* dr = st.in(0, rhs, n);
    double* dx = st.inout(1, x, n, false);
    h.coarse_solve(dr, dx);
    st.out(1, x, n);
    st.finish();
  });
}

int amgx_n_levels(amgx_handle h) { return (h && h->h) ? h->h->n_levels() : 0; }

int amgx_level_info(amgx_handle hh, int level, int64_t* n, int32_t* bs, int64_t* nnz) {
  return guard(hh, [&](amgx::Handle& h) {
    if (level < 0 || level >= h.n_levels()) throw amgx::Err("amgx_level_info: level out of range");
    if (n) *n = h.lev[level].n;
    if (bs) *bs = h.lev[level].bs;
    if (nnz) *nnz = h.lev[level].A.nnz;
  });
}

int amgx_cycle_info(amgx_handle hh, int32_t* tail_level, int32_t* dense_level, int64_t* dense_n) {
  return guard(hh, [&](amgx::Handle& h) {
    if (tail_level) *tail_level = h.dense_level >= 0 ? -1 : h.tail_level;
    if (dense_level) *dense_level = h.dense_level;
    if (dense_n) *dense_n = h.dense_level >= 0 ? h.dense_n : 0;
  });
}

int amgx_matrix_info(amgx_handle hh, int level, int which, int32_t* fmt, int64_t* stored, int32_t* lanes) {
  return guard(hh, [&](amgx::Handle& h) {
    if (level < 0 || level >= h.n_levels()) throw amgx::Err("amgx_matrix_info: level out of range");
    if (which < 0 || which > 7) throw amgx::Err("matrix query: which must be 0..7");
    const amgx::DevLevel& LV = h.lev[level];
    if (which == 7) {                         // the single-precision image of A: the format, entries and lanes of A itself
      const amgx::DevMatrix& M = LV.A;
      if (fmt) *fmt = M.has32() ? M.fmt : -1;
      if (stored) *stored = M.has32() ? M.stored : 0;
      if (lanes) *lanes = M.has32() ? M.lanes : 0;
      return;
    }
    if (which == 3 && LV.dia.on()) {          // the symmetric diagonal image of A stands in for A' (format 6)
      if (fmt) *fmt = 6;
      if (stored) *stored = (int64_t)LV.dia.K * LV.n;
      if (lanes) *lanes = 1;
      return;
    }
    const amgx::DevMatrix& M = which == 0 ? LV.A : which == 1 ? LV.P : which == 2 ? LV.PT : which == 3 ? LV.Apre : which == 4 ? LV.Q : which == 5 ? LV.ApreLW : LV.QLW;
    if (fmt) *fmt = M.empty() ? -1 : (which >= 5 ? 5 : ((M.fmt == amgx::FMT_SELL && M.sell.win) ? 3 : M.fmt));
    if (stored) *stored = M.stored;
    if (lanes) *lanes = M.lanes;
  });
}

int amgx_matrix_stream_bytes(amgx_handle hh, int level, int which, int64_t* bytes) {
  return guard(hh, [&](amgx::Handle& h) {
    if (level < 0 || level >= h.n_levels() || !bytes) throw amgx::Err("amgx_matrix_stream_bytes: bad arguments");
    if (which < 0 || which > 7) throw amgx::Err("matrix query: which must be 0..7");
    const amgx::DevLevel& LV = h.lev[level];
    // single-precision image of A: the indices and pointers of A + 4 bytes per stored value (0: not built)
    if (which == 7) { *bytes = LV.A.has32() ? LV.A.stream_bytes32() : 0; return; }
    // diagonal image: the K upper diagonals (the lower ones are re-reads of the same arrays) + the dinv stream the kernel reads in
    // place of the wdiag slot
    if (which == 3 && LV.dia.on()) { *bytes = (int64_t)(LV.dia.K + 1) * LV.n * (int64_t)sizeof(double); return; }
    const amgx::DevMatrix& M = which == 0 ? LV.A : which == 1 ? LV.P : which == 2 ? LV.PT : which == 3 ? LV.Apre : which == 4 ? LV.Q : which == 5 ? LV.ApreLW : LV.QLW;
    *bytes = M.stream_bytes;
  });
}

int amgx_level_paths(amgx_handle hh, int level, int64_t* out, int n_out) {
  return guard(hh, [&](amgx::Handle& h) {
    if (level < 0 || level >= h.n_levels()) throw amgx::Err("amgx_level_paths: level out of range");
    if (!out || n_out < 1) throw amgx::Err("amgx_level_paths: bad arguments");
    const amgx::DevLevel& L = h.lev[level];
    const amgx::DevRestrict& R = L.RF;
    int64_t v[AMGX_LEVEL_PATHS_N] = {};
    const int down = L.paths.down;
    const amgx::DownPlan& plan = L.plan_rf;
    if (plan.on) {                        // (the fused block-hybrid form has a plan of its own: entry 33)
      v[0] = down == amgx::DOWN_DIA_BOX ? (int)amgx::DOWN_DIA : down;
      v[1] = plan.threads;
      v[2] = plan.lanes;
      v[3] = plan.ept;
      v[18] = plan.n_chunks;
    }
    if (!R.empty()) {
      v[4] = R.boxed ? 2 : R.slice_list.n ? 1 : 0;
      v[5] = R.max_slots;
      v[6] = R.max_entries;
    }
    v[7] = L.dia.K;
    v[8] = L.A.sell.xcd; v[9] = L.Apre.sell.xcd; v[10] = L.Q.sell.xcd; v[11] = L.dia.xcd;
    auto slices = [](const amgx::DevMatrix& M, int64_t* c16, int64_t* all) {
      if (M.empty() || M.fmt != amgx::FMT_SELL || M.n_slices <= 0) return;
      const std::vector<int64_t> sp = amgx::db_download(M.sell.slice_ptr, (size_t)M.n_slices);
      *all = M.n_slices;
      for (int64_t p : sp) *c16 += p & 1;
    };
    slices(L.A, &v[12], &v[13]);
    slices(L.Apre, &v[14], &v[15]);
    if (!L.ApreLW.empty() && L.lw_cptr.n > 1) {
      const std::vector<int32_t> cp = amgx::db_download(L.lw_cptr, L.lw_cptr.n);
      for (size_t c = 0; c + 1 < cp.size(); ++c) v[16] += cp[c + 1] == cp[c];
    }
    v[17] = L.paths.folded ? 1 : 0;
    const amgx::DevGS& gs = L.gs;
    const amgx::DevGSB& gsb = L.gsb;
    const amgx::DevBGSB& bgsb = L.bgsb;
    v[19] = L.paths.sweep;
    switch (L.paths.sweep) {
      case amgx::SWEEP_BGS: {
        v[23] = L.bgs.n_colors;
        const amgx::BgsShape sh = amgx::bgs_block_shape(L.A.n_rows ? (double)L.A.nnz / (double)L.A.n_rows : 0.0, L.bgs.max_m);
        v[34] = sh.TH; v[35] = sh.G; v[36] = L.bgs.max_m;
        break;
      }
      case amgx::SWEEP_BGSB:
      case amgx::SWEEP_BGSB_BC:
        v[21] = amgx::BLOCK; v[22] = bgsb.BB; v[23] = bgsb.n_colors; v[24] = bgsb.n_bcolors; v[25] = bgsb.has_split;
        break;
      case amgx::SWEEP_GSB:
        v[20] = gsb.G; v[21] = gsb.TH; v[22] = gsb.B; v[23] = gsb.n_colors; v[25] = gsb.has_split;
        v[26] = gsb.lowin_maxw; v[27] = gsb.full_maxw;
        v[28] = gsb.has_split && gsb.narrow;
        v[29] = gsb.mid;
        v[30] = gsb.lw;
        v[32] = gsb.has_fullLW ? gsb.flw_no_window : 0;
        // (the form residual_restrict_after_zero picks; only where the cycle's down pass runs it)
        if (down == amgx::DOWN_GSB) v[33] = L.plan_rg.family == amgx::DOWN_FAM_LW ? 3 : L.plan_rg.family == amgx::DOWN_FAM_WIN ? 2 : 1;
        break;
      case amgx::SWEEP_MC: v[20] = gs.lanes; v[21] = amgx::BLOCK; v[23] = gs.n_colors; v[25] = gs.has_split; break;
      case amgx::SWEEP_MC_BSELL: v[21] = amgx::BLOCK; v[23] = gs.n_colors; v[25] = gs.bsplit; break;
      case amgx::SWEEP_MC_ROWLIST: {
        v[21] = amgx::BLOCK; v[23] = gs.n_colors;
        const double avg = L.A.n_rows ? (double)L.A.nnz / (double)L.A.n_rows : 0.0;
        for (int c = 0; c < gs.n_colors; ++c) {
          const int64_t rows = gs.color_row_ptr[c + 1] - gs.color_row_ptr[c];
          if (rows > 0) v[31] |= amgx::bgs_rowlist_w(avg, rows);
        }
        break;
      }
      default: break;
    }
    auto bcsr = [](const amgx::DevMatrix& M) -> int64_t {
      if (M.empty() || M.fmt != amgx::FMT_CSRVEC || (M.br == 1 && M.bc == 1)) return 0;
      const amgx::BcsrKernel bk = amgx::bcsr_kernel(M, false);
      return (bk.rowlane ? 100 : 200) + bk.width;
    };
    v[37] = bcsr(L.A); v[38] = bcsr(L.P); v[39] = bcsr(L.PT);
    for (int k = 0; k < std::min(n_out, AMGX_LEVEL_PATHS_N); ++k) out[k] = v[k];
  });
}

int amgx_level_extra(amgx_handle hh, int level, int64_t* out, int n_out) {
  return guard(hh, [&](amgx::Handle& h) {
    if (level < 0 || level >= h.n_levels()) throw amgx::Err("amgx_level_extra: level out of range");
    if (!out || n_out < 1) throw amgx::Err("amgx_level_extra: bad arguments");
    const amgx::DevLevel& L = h.lev[level];
    const bool tail = h.dense_level < 0 && h.tail_level > 0;
    int64_t v[AMGX_LEVEL_EXTRA_N] = {};
    v[0] = tail ? h.tail_ops : 0;
    v[1] = tail && level >= h.tail_level && level < (int)h.tail_gs_lds.size() ? h.tail_gs_lds[level] : -1;
    if (L.paths.sweep == amgx::SWEEP_MC && L.gs.n_slices_total > 0) {
      const amgx::DevMatrix::Sell* img[3] = {&L.gs.sell, L.gs.has_split ? &L.gs.lower : nullptr, L.gs.has_split ? &L.gs.upper : nullptr};
      for (const amgx::DevMatrix::Sell* S : img) {
        if (!S) continue;
        const std::vector<int64_t> sp = amgx::db_download(S->slice_ptr, (size_t)L.gs.n_slices_total);
        for (int64_t p : sp) v[2] += p & 1;
        v[3] += L.gs.n_slices_total;
      }
      v[4] = L.gs.sell.rowrel;
    }
    if (!L.A.empty() && L.A.fmt == amgx::FMT_SELL) v[5] = L.A.sell.diag_first;
    if (!L.Apre.empty() && L.Apre.fmt == amgx::FMT_SELL) { v[6] = L.Apre.sell.diag_first; v[7] = L.Apre.sell.wdiag; }
    v[8] = (int64_t)h.graphs.size();
    v[9] = L.gs32 ? 1 : 0; v[10] = L.gs32_images; v[11] = L.gs32_bytes;
    // (a scalar Gauss-Seidel level with single-precision images, DESIGN.md 5.21: the same three meanings)
    if (L.sgs32 || L.sgs32_wide) { v[9] = L.sgs32 ? 1 : 0; v[10] = __builtin_popcount((unsigned)L.sgs_mask); v[11] = L.sgs_bytes; }
    for (int k = 0; k < std::min(n_out, AMGX_LEVEL_EXTRA_N); ++k) out[k] = v[k];
  });
}

int amgx_jacobi_prec_info(amgx_handle hh, int level, int64_t* out, int n_out) {
  return guard(hh, [&](amgx::Handle& h) {
    if (level < 0 || level >= h.n_levels()) throw amgx::Err("amgx_jacobi_prec_info: level out of range");
    if (!out || n_out < 1) throw amgx::Err("amgx_jacobi_prec_info: bad arguments");
    const amgx::DevLevel& L = h.lev[level];
    const int64_t v[AMGX_JACOBI_PREC_INFO_N] = {L.jp32 ? 1 : 0, L.jp_mask, L.jp_bytes, L.jp_released, L.jp32_wide ? 1 : 0};
    for (int k = 0; k < std::min(n_out, AMGX_JACOBI_PREC_INFO_N); ++k) out[k] = v[k];
  });
}

int amgx_gs_prec_info(amgx_handle hh, int level, int64_t* out, int n_out) {
  return guard(hh, [&](amgx::Handle& h) {
    if (level < 0 || level >= h.n_levels()) throw amgx::Err("amgx_gs_prec_info: level out of range");
    if (!out || n_out < 1) throw amgx::Err("amgx_gs_prec_info: bad arguments");
    const amgx::DevLevel& L = h.lev[level];
    const int64_t v[AMGX_GS_PREC_INFO_N] = {L.sgs32 ? 1 : 0, L.sgs_mask, L.sgs_bytes, L.sgs_released, L.sgs32_wide ? 1 : 0};
    for (int k = 0; k < std::min(n_out, AMGX_GS_PREC_INFO_N); ++k) out[k] = v[k];
  });
}

int amgx_time_op(amgx_handle hh, int level, int op, int reps, double* avg_ms) {
  return guard(hh, [&](amgx::Handle& h) {
    if (level < 0 || level >= h.n_levels()) throw amgx::Err("amgx_time_op: level out of range");
    if (reps < 1 || !avg_ms) throw amgx::Err("amgx_time_op: bad arguments");
    amgx::DevLevel& L = h.lev[level];
    const bool has_c = level + 1 < h.n_levels();
    if ((op == 2 || op == 3 || op == 5 || op == 6 || op == 7) && !has_c) throw amgx::Err("amgx_time_op: no transfer on the coarsest level");
    if (op == 1 && (!L.dinv.p || L.sm_type != AMGX_SM_JACOBI)) throw amgx::Err("amgx_time_op: level has no Jacobi smoother");
    if (op == 10 && (!L.dinv.p || L.sm_type != AMGX_SM_CHEBY || !L.d.p || L.cheb_degree < 1)) throw amgx::Err("amgx_time_op: level has no Chebyshev smoother");
    auto launch = [&]() {
      switch (op) {
        case 0: h.residual(L.A, L.x.p, L.rhs.p, L.res.p); break;
        case 1: h.jacobi_fused(L, L.tmp.p, L.rhs.p, L.x.p); break;
        case 10: h.cheb_step(L, L.tmp.p, L.rhs.p, L.x.p, L.cheb_c1[2], L.cheb_c2[2], L.d.p, L.d.p); break;   // a middle step: reads and stores d
        case 2: h.transfer_f2c(level, L.res.p, h.lev[level + 1].rhs.p); break;
        case 3: h.mult_add(L.P, 1.0, h.lev[level + 1].x.p, L.x.p, L.tmp.p); break;
        case 4: h.run_cycle(h.lev[0].x.p, h.lev[0].rhs.p, true); break;
        case 5: h.pre_smooth_restrict(level, L.x.p, L.rhs.p, L.res.p, h.lev[level + 1].rhs.p, h.folded(L)); break;
        case 6: h.post_smooth(level, L.x.p, L.rhs.p, L.res.p, h.lev[level + 1].x.p, h.folded(L)); break;
        case 7:
          if (!L.plan_rf.on) throw amgx::Err("amgx_time_op: level has no fused pre-smoothing + restriction kernel");
          h.skip_rsum = true;
          try { h.pre_smooth_restrict(level, L.x.p, L.rhs.p, L.res.p, h.lev[level + 1].rhs.p, h.folded(L)); } catch (...) { h.skip_rsum = false; throw; }
          h.skip_rsum = false;
          break;
        default: throw amgx::Err("amgx_time_op: unknown op");
      }
    };
    // op 11: a square-block Gauss-Seidel level that the V-cycle sweeps with separate launches (not folded, not collapsed)
    const int sw = L.paths.sweep;
    const bool block_sweep_in_cycle = has_c && L.paths.plain && L.sm_type == AMGX_SM_GS && L.bs > 1 && L.n == L.ncols && !L.paths.folded &&
                                      (L.paths.bgsb() || sw == amgx::SWEEP_MC_BSELL || sw == amgx::SWEEP_MC_ROWLIST) &&
                                      h.cycle == AMGX_CYCLE_V && (h.dense_level < 0 || level < h.dense_level);
    if (op == 8 || op == 9 || op == 11) {
      // the dominant kernel timed where it runs: inside the cycle, between the previous cycle's last kernel and the
      // partial-sum reduction (cache state and clocks of the real application), averaged over `reps` cycles
      if (op == 8 && !(L.plan_rf.on && L.plan_rf.mode == 0)) throw amgx::Err("amgx_time_op: level has no fused pre-smoothing + restriction kernel");
      if (op == 9 && !(has_c && L.paths.plain && L.paths.hybrid() && L.n == L.ncols && !L.paths.folded))
        throw amgx::Err("amgx_time_op: level has no block-hybrid Gauss-Seidel sweep");
      if (op == 11 && !block_sweep_in_cycle)
        throw amgx::Err("amgx_time_op: level has no block Gauss-Seidel sweep in the cycle");
      if (h.stream == nullptr) throw amgx::Err("amgx_time_op: ops 8, 9 and 11 need a non-default stream");
      amgx::Handle::ProbeScope probe(h, op);
      double tot = 0.0;
      if (h.lev[0].len()) amgx::launch(amgx::fill_kernel, amgx::Handle::grid_for(h.lev[0].len()), amgx::BLOCK, 0, h.stream, h.lev[0].len(), (uint64_t)2, h.lev[0].rhs.p);
      h.do_cycle(h.lev[0].x.p, h.lev[0].rhs.p);              // warm-up
      h.probe_level = level;
      for (int i = 0; i < reps; ++i) {
        h.do_cycle(h.lev[0].x.p, h.lev[0].rhs.p);
        HIPCHK(hipEventSynchronize(h.probe_e1));
        tot += probe.elapsed_ms();
      }
      HIPCHK(hipStreamSynchronize(h.stream));
      *avg_ms = tot / reps;
      return;
    }
    if (op != 4) {   // time on non-trivial data (the work vectors are otherwise zero in device-pointer mode)
      auto fill = [&](double* v, int64_t n, uint64_t seed) {
        if (n) amgx::launch(amgx::fill_kernel, amgx::Handle::grid_for(n), amgx::BLOCK, 0, h.stream, n, seed, v);
      };
      fill(L.x.p, L.len(), 1); fill(L.rhs.p, L.len(), 2); fill(L.res.p, L.len(), 3); fill(L.tmp.p, L.len(), 4);
      if (has_c) fill(h.lev[level + 1].x.p, h.lev[level + 1].len(), 5);
    }
    hipEvent_t e0, e1;
    HIPCHK(hipEventCreate(&e0));
    HIPCHK(hipEventCreate(&e1));
    launch();                                    // warm-up (and graph capture for op 4)
    HIPCHK(hipStreamSynchronize(h.stream));
    HIPCHK(hipEventRecord(e0, h.stream));
    for (int i = 0; i < reps; ++i) launch();
    HIPCHK(hipEventRecord(e1, h.stream));
    HIPCHK(hipEventSynchronize(e1));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    *avg_ms = (double)ms / reps;
  });
}

int amgx_smoother_info(amgx_handle hh, int level, int32_t* sm_type, int32_t* degree, double* lambda_max, double* lambda_min, int32_t* estimated) {
  return guard(hh, [&](amgx::Handle& h) {
    if (level < 0 || level >= h.n_levels()) throw amgx::Err("amgx_smoother_info: level out of range");
    const amgx::DevLevel& L = h.lev[level];
    const bool ch = L.sm_type == AMGX_SM_CHEBY;
    if (sm_type) *sm_type = L.sm_type;
    if (degree) *degree = ch ? L.cheb_degree : 0;
    if (lambda_max) *lambda_max = ch ? L.cheb_lmax : 0.0;
    if (lambda_min) *lambda_min = ch ? L.cheb_lmin : 0.0;
    if (estimated) *estimated = ch ? L.cheb_estimated : 0;
  });
}

}  // extern "C"

#include "krylov.hpp"

namespace amgx {
// lambda_max(Dinv A) of the Chebyshev levels that got none: power iteration with the Rayleigh quotient in the A inner product,
//   v_0 = Dinv A f (f = fill_kernel(seed 1): non-free rows become zero),   t = A v,  w = Dinv t,  lambda = <t, w> / <t, v>,  v <- w / lambda
// 30 steps, lmax = 1.1 x the last lambda.  For symmetric positive semi-definite A and Dinv the quotient equals
// <u, A^1/2 Dinv A^1/2 u> / <u, u> with u = A^1/2 v, so it never exceeds lambda_max.  Deterministic reductions (kr_dot_*).
static void cheb_estimate(Handle& h) {
  DevBuf<double> partial, sc;
  for (int l = 0; l < h.n_levels(); ++l) {
    DevLevel& L = h.lev[l];
    if (L.sm_type != AMGX_SM_CHEBY || L.cheb_lmax > 0.0) continue;
    const int64_t n = L.len();
    if (n == 0 || !L.dinv.p || L.A.empty()) { L.cheb_set_interval(1.0); L.cheb_estimated = 1; continue; }
    if (!partial.p) { partial.alloc((size_t)2 * KR_BLOCKS); sc.alloc(2); }
    const int nb = (int)std::max<int64_t>(1, std::min<int64_t>(KR_BLOCKS, (n + BLOCK - 1) / BLOCK));
    double *v = L.x.p, *t = L.res.p, *w = L.tmp.p;
    launch(fill_kernel, Handle::grid_for(n), BLOCK, 0, h.stream, n, (uint64_t)1, w);
    h.mult(L.A, w, t);
    h.cheb_first(L, t, nullptr, v, nullptr, 1.0);
    double lam = 0.0;
    for (int it = 0; it < 30; ++it) {
      h.mult(L.A, v, t);
      h.cheb_first(L, t, nullptr, w, nullptr, 1.0);
      launch(kr_dot_partial_kernel, nb, BLOCK, 0, h.stream, n, (const double*)t, (const double*)w, partial.p);
      launch(kr_dot_partial_kernel, nb, BLOCK, 0, h.stream, n, (const double*)t, (const double*)v, partial.p + KR_BLOCKS);
      launch(kr_dot_final_kernel, 2, BLOCK, 0, h.stream, nb, (const double*)partial.p, sc.p);
      double two[2] = {0.0, 0.0};
      HIPCHK(hipMemcpyAsync(two, sc.p, 2 * sizeof(double), hipMemcpyDeviceToHost, h.stream));
      HIPCHK(hipStreamSynchronize(h.stream));
      if (!(two[1] > 0.0) || !(two[0] > 0.0) || !std::isfinite(two[0] / two[1])) break;      // A v = 0 (no free row): keep the last value
      lam = two[0] / two[1];
      launch(kr_scale_kernel, Handle::grid_for(n), BLOCK, 0, h.stream, n, 1.0 / lam, (const double*)w, v, 0);
    }
    if (!(lam > 0.0)) lam = 1.0;
    L.cheb_set_interval(1.1 * lam);
    L.cheb_estimated = 1;
    const size_t len = (size_t)std::max<int64_t>(1, L.ext_len());
    for (double* q : {L.x.p, L.res.p, L.tmp.p}) HIPCHK(hipMemsetAsync(q, 0, len * sizeof(double), h.stream));
    HIPCHK(hipStreamSynchronize(h.stream));
  }
}
}  // namespace amgx

#include "multi.hpp"
#include "mv_kernels.hpp"      // Gram matrix and combination of multi-vectors
#include "mv.hpp"
#include "dist.hpp"
#include "gss4.hpp"
