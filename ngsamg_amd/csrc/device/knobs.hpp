// Every environment switch of the device library, once.  Knobs::from_env() is the only place under csrc/device that reads the
// environment (exceptions: AMGX_ROCTX in amgx.hip, NGSAMG_RCCL_LIB in dist.hpp and OMP_NUM_THREADS in the two host helpers of
// amgx.hip, which are process-wide and predate any handle).  It runs once per amgx_create / amgx_dist_create / amgx_comm_create on
// the calling thread, before any SetupTasks worker starts -- tests change the environment between two creates of one process --
// and the result is stored in the Handle (the Comm), where everything that needs a switch later finds it.
//
// Kinds:  kill switch = turns a default path off;  threshold = moves a size rule;  test hook = forces a rarely taken path for the
// suite;  A/B hook = opt-in path with a recorded measurement (see the comment at the place that uses it).
#pragma once
#include "../../../include/amgx.h"
#include "down_plan.hpp"       // DownSizes, DOWN_THREADS
#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <thread>

namespace amgx {

// entry counts and column indices on the device are 32-bit
static constexpr int64_t I32_MAX = 2147483647;

struct Knobs {
  // ---- setup (amgx_create) itself
  bool setup_log = false;               // AMGX_SETUP_LOG: wall-clock time of the stages and tasks of amgx_create on stderr (test hook)
  bool setup_serial = false;            // AMGX_SETUP_SERIAL: the host tasks of a level run one after the other (test hook)
  int setup_threads = 1;                // AMGX_SETUP_THREADS: host threads of the format builders; default min(cores, 32) (threshold)
  bool verify_images = false;           // AMGX_VERIFY_IMAGES: every device-built image is compared with the host builder's (test hook)
  bool host_images = false;             // AMGX_HOST_IMAGES: no device builders at all (kill switch)
  int64_t dev_images_min_rows = 65536;  // AMGX_DEV_IMAGES_MIN_ROWS: smallest level whose images are built on the device (threshold)
  bool host_lw = false;                 // AMGX_HOST_LW: the local-window images come from the host builder (kill switch)
  bool gs_perm = false;                 // AMGX_GS_PERM: colour-major renumbering of Gauss-Seidel levels (A/B hook)
  // ---- matrix formats
  int sell_max_lanes = 0;               // AMGX_SELL_MAX_LANES: cap on the lanes per row of a SELL image (1, 2, 4, 8, 16), 0 = none (test hook)
  int sell_long_row_lanes = 1;          // AMGX_SELL_LONG_ROW_LANES: least lanes per row (1, 2, 4, 8, 16) for rows of >= 24 entries (A/B hook)
  bool no_sell_window = false;          // AMGX_NO_SELL_WINDOW: no length-sorted windows (kill switch)
  bool no_sell_window_short = false;    // AMGX_NO_SELL_WINDOW_SHORT: no windowed fallback for short ragged rows (kill switch)
  bool no_diag_first = false;           // AMGX_NO_DIAG_FIRST: CSR entry order instead of diagonal first (kill switch)
  bool no_bsell = false;                // AMGX_NO_BSELL: square-block matrices stay in block CSR (kill switch)
  int bsell_xmode = 0;                  // AMGX_BSELL_XMODE: gathered-vector access of the BSELL kernels, 0 .. 5 (A/B hook)
  bool no_rb_transfer = false;          // AMGX_NO_RB_TRANSFER: block transfers never take the rigid-body form (kill switch)
  int xcd = 1;                          // AMGX_XCD: workgroup -> rows mapping, 0 off / 1 long-row levels / 2 all / 3 + transfers (A/B hook)
  bool dia_xcd = false;                 // AMGX_DIA_XCD: each XCD walks one contiguous eighth of the diagonal image's chunks (A/B hook)
  // ---- Jacobi down pass: A', the diagonal image, the local-window image, the fused restriction
  bool no_wdiag = false;                // AMGX_NO_WDIAG: the diagonal slot of A' keeps A'_ii (kill switch)
  bool apre_window = false;             // AMGX_APRE_WINDOW: windowed A' on levels >= 1 (A/B hook)
  bool no_dia = false;                  // AMGX_NO_DIA: no symmetric diagonal image (kill switch)
  int64_t dia_min_rows = 2000000;       // AMGX_DIA_MIN_ROWS: smallest level that takes the diagonal image (threshold)
  double dia_max_fill = 1.05;           // AMGX_DIA_MAX_FILL: stored / present entries up to which a level takes the diagonal image (threshold)
  bool no_dia_box = false;              // AMGX_NO_DIA_BOX: the diagonal image keeps its chunks of 512 consecutive rows (kill switch)
  int64_t dia_box_min_rows = 200000;    // AMGX_DIA_BOX_MIN_ROWS: smallest grid level whose diagonal image takes box chunks (threshold)
  int dia_box_yc = 0, dia_box_zc = 0;   // AMGX_DIA_BOX_SHAPE=YxZ: grid lines per box in y and z; default 2x4 in 3D, 8x1 in 2D (A/B hook)
  bool no_lw = false;                   // AMGX_NO_LW: no local-window images (kill switch)
  bool no_qlw = false;                  // AMGX_NO_QLW: no local-window image of Q (kill switch)
  int64_t lw_min_rows = 100000;         // AMGX_LW_MIN_ROWS: smallest level that takes local-window images (threshold)
  bool lw_test_cap_on = false;          // AMGX_LW_TEST_CAP: a smaller window capacity sends some chunks through the no-window path
  int64_t lw_test_cap = 0;              //   (test hook)
  bool no_fused_restrict = false;       // AMGX_NO_FUSED_RESTRICT: separate smoothing and restriction kernels (kill switch)
  bool no_fused_restrict_multi = false; // AMGX_NO_FUSED_RESTRICT_MULTI: ... on images with several lanes per row only (kill switch)
  bool cheb_no_fused_restrict = false;  // AMGX_CHEB_NO_FUSED_RESTRICT: ... on Chebyshev levels only (kill switch)
  int fused_block = DOWN_THREADS;               // AMGX_FUSED_BLOCK: workgroup size of the fused down kernel, 256 / 512 / 1024 (A/B hook)
  int fused_ept_max = INT_MAX;          // AMGX_FUSED_EPT_MAX: chunks with more entries of P per thread keep the separate kernels (A/B hook)
  bool rsum_sort = false;               // AMGX_RSUM_SORT: partial sums stored row by row (A/B hook)
  bool no_compact_chunks = false;       // AMGX_NO_COMPACT_CHUNKS: consecutive chunks only (kill switch)
  int64_t compact_chunks_min_rows = 200000;   // AMGX_COMPACT_CHUNKS_MIN_ROWS: smallest level with compact chunks (threshold)
  int64_t restrict_min_rows = INT64_MAX;      // AMGX_RESTRICT_MIN_ROWS: smallest level with the column-blocked restriction (A/B hook)
  // ---- folded prolongation
  bool no_fold = false;                 // AMGX_NO_FOLD: the literal post-smoothing sequence (kill switch)
  bool no_block_fold = false;           // AMGX_NO_BLOCK_FOLD: ... on block levels only (kill switch)
  double q_max_pad = 1.6;               // AMGX_Q_MAX_PAD: padding up to which Q takes a SELL image (threshold)
  // ---- Gauss-Seidel
  bool gs_rowrel = false;               // AMGX_GS_ROWREL: row-relative 16-bit columns in the colour-major copy (A/B hook)
  int64_t bgs_bsell_min = 4096;         // AMGX_BGS_BSELL_MIN: rows per colour from which block levels get a BSELL copy (test hook)
  bool no_bgs_bsell = false;            // AMGX_NO_BGS_BSELL: block levels keep the CSR row-list kernel (kill switch)
  bool no_bgs_split = false;            // AMGX_NO_BGS_SPLIT: no lower / upper split copies on block levels (kill switch)
  bool gsb_lw = false;                  // AMGX_GSB_LW: local-window image of the block-hybrid sweep (A/B hook)
  bool gsb_no_split = false;            // AMGX_GSB_NO_SPLIT: block-hybrid levels without the lower / rest split (kill switch)
  bool gsb_no_narrow = false;           // AMGX_GSB_NO_NARROW: the sweep from zero takes the general kernel (kill switch)
  bool gsb_no_mid = false;              // AMGX_GSB_NO_MID: the general sweep never takes the mid-width kernel (kill switch)
  bool bgsb_no_split = false;           // AMGX_BGSB_NO_SPLIT: square-block hybrid levels without the split (kill switch)
  // ---- single-precision matrix images (Chebyshev levels, Gauss-Seidel block levels)
  bool no_mat_f32 = false;              // AMGX_NO_MAT_F32: mat_prec = AMGX_PREC_F32 is ignored, no single-precision image (kill switch)
  bool gs_f32_wide = false;             // AMGX_GS_F32_WIDE: Gauss-Seidel levels keep fp64 images that hold the rounded values (A/B hook)
  // ---- epilogues, coarse end of the cycle
  bool no_ep_nt = false;                // AMGX_NO_EP_NT: no non-temporal epilogue operands (kill switch)
  bool no_ep_hoist = false;             // AMGX_NO_EP_HOIST: epilogue operands are not loaded ahead of the row product (kill switch)
  bool no_dense_tail = false;           // AMGX_NO_DENSE_TAIL: no collapsed coarse levels (kill switch)
  int64_t dense_max = 8192;             // AMGX_DENSE_MAX: largest level that may collapse into the dense operator (threshold)
  int64_t coarse_dense_max = 16384;     // AMGX_COARSE_DENSE_MAX: largest coarsest level inverted on the device (threshold)
  bool no_tail_kernel = false;          // AMGX_NO_TAIL_KERNEL: no single-workgroup coarse tail (kill switch)
  bool no_tail_lds = false;             // AMGX_NO_TAIL_LDS: its Gauss-Seidel sweeps keep x in global memory (kill switch)
  // ---- rank-partitioned hierarchies (dist.hpp)
  bool dist_events = false;             // AMGX_DIST_EVENTS: cross-stream ordering by events, not by device flags (kill switch)
  bool dist_graph = true;               // AMGX_DIST_GRAPH=0: direct launches instead of the whole-cycle graph (kill switch)
  bool dist_no_overlap = false;         // AMGX_DIST_NO_OVERLAP: no interior / boundary split around the halo exchange (kill switch)
  int dist_force_allgather = 0;         // AMGX_DIST_FORCE_ALLGATHER: world size 1 through ncclAllGather (1), "pad": padded (2) (test hook)
  bool dist_tail_graph = false;         // AMGX_DIST_TAIL_GRAPH: the replicated tail replays a graph of its own (A/B hook)

  static Knobs from_env() {
    Knobs k;
    auto on = [](const char* name) { return std::getenv(name) != nullptr; };
    auto i64 = [](const char* name, int64_t& v) { if (const char* e = std::getenv(name)) v = std::atoll(e); };
    k.setup_log = on("AMGX_SETUP_LOG");
    k.setup_serial = on("AMGX_SETUP_SERIAL");
    k.setup_threads = (int)std::min<unsigned>(std::max(1u, std::thread::hardware_concurrency()), 32u);
    if (const char* e = std::getenv("AMGX_SETUP_THREADS")) k.setup_threads = std::max(1, std::atoi(e));
    k.verify_images = on("AMGX_VERIFY_IMAGES");
    k.host_images = on("AMGX_HOST_IMAGES");
    i64("AMGX_DEV_IMAGES_MIN_ROWS", k.dev_images_min_rows);
    k.host_lw = on("AMGX_HOST_LW");
    k.gs_perm = on("AMGX_GS_PERM");
    // lanes per row: the SELL kernels exist for G in {1, 2, 4, 8, 16} (R = WAVE / G rows per wave), so any other value is rounded
    // down to the next of them (3 -> 2, 100 -> 16, 0 and negative values -> 1)
    auto lanes = [](const char* e) { const int v = std::atoi(e); int g = 1; while (g < 16 && 2 * g <= v) g *= 2; return g; };
    if (const char* e = std::getenv("AMGX_SELL_MAX_LANES")) k.sell_max_lanes = lanes(e);
    if (const char* e = std::getenv("AMGX_SELL_LONG_ROW_LANES")) k.sell_long_row_lanes = lanes(e);
    k.no_sell_window = on("AMGX_NO_SELL_WINDOW");
    k.no_sell_window_short = on("AMGX_NO_SELL_WINDOW_SHORT");
    k.no_diag_first = on("AMGX_NO_DIAG_FIRST");
    k.no_bsell = on("AMGX_NO_BSELL");
    if (const char* e = std::getenv("AMGX_BSELL_XMODE")) k.bsell_xmode = std::max(0, std::min(5, std::atoi(e)));
    k.no_rb_transfer = on("AMGX_NO_RB_TRANSFER");
    if (const char* e = std::getenv("AMGX_XCD")) k.xcd = std::atoi(e);
    k.dia_xcd = on("AMGX_DIA_XCD");
    k.no_wdiag = on("AMGX_NO_WDIAG");
    k.apre_window = on("AMGX_APRE_WINDOW");
    k.no_dia = on("AMGX_NO_DIA");
    i64("AMGX_DIA_MIN_ROWS", k.dia_min_rows);
    if (const char* e = std::getenv("AMGX_DIA_MAX_FILL")) k.dia_max_fill = std::max(1.0, std::atof(e));
    k.no_dia_box = on("AMGX_NO_DIA_BOX");
    i64("AMGX_DIA_BOX_MIN_ROWS", k.dia_box_min_rows);
    if (const char* e = std::getenv("AMGX_DIA_BOX_SHAPE")) {
      int y = 0, z = 0;
      if (std::sscanf(e, "%dx%d", &y, &z) == 2 && y > 0 && z > 0) { k.dia_box_yc = y; k.dia_box_zc = z; }
    }
    k.no_lw = on("AMGX_NO_LW");
    k.no_qlw = on("AMGX_NO_QLW");
    i64("AMGX_LW_MIN_ROWS", k.lw_min_rows);
    k.lw_test_cap_on = on("AMGX_LW_TEST_CAP");
    i64("AMGX_LW_TEST_CAP", k.lw_test_cap);
    k.no_fused_restrict = on("AMGX_NO_FUSED_RESTRICT");
    k.no_fused_restrict_multi = on("AMGX_NO_FUSED_RESTRICT_MULTI");
    k.cheb_no_fused_restrict = on("AMGX_CHEB_NO_FUSED_RESTRICT");
    if (const char* e = std::getenv("AMGX_FUSED_BLOCK")) { const int v = std::atoi(e); k.fused_block = contains(DownSizes{}, v) ? v : DOWN_THREADS; }
    if (const char* e = std::getenv("AMGX_FUSED_EPT_MAX")) k.fused_ept_max = std::atoi(e);
    k.rsum_sort = on("AMGX_RSUM_SORT");
    k.no_compact_chunks = on("AMGX_NO_COMPACT_CHUNKS");
    i64("AMGX_COMPACT_CHUNKS_MIN_ROWS", k.compact_chunks_min_rows);
    i64("AMGX_RESTRICT_MIN_ROWS", k.restrict_min_rows);
    k.no_fold = on("AMGX_NO_FOLD");
    k.no_block_fold = on("AMGX_NO_BLOCK_FOLD");
    if (const char* e = std::getenv("AMGX_Q_MAX_PAD")) k.q_max_pad = std::atof(e);
    k.gs_rowrel = on("AMGX_GS_ROWREL");
    i64("AMGX_BGS_BSELL_MIN", k.bgs_bsell_min);
    k.no_bgs_bsell = on("AMGX_NO_BGS_BSELL");
    k.no_bgs_split = on("AMGX_NO_BGS_SPLIT");
    k.gsb_lw = on("AMGX_GSB_LW");
    k.gsb_no_split = on("AMGX_GSB_NO_SPLIT");
    k.gsb_no_narrow = on("AMGX_GSB_NO_NARROW");
    k.gsb_no_mid = on("AMGX_GSB_NO_MID");
    k.bgsb_no_split = on("AMGX_BGSB_NO_SPLIT");
    k.no_mat_f32 = on("AMGX_NO_MAT_F32");
    k.gs_f32_wide = on("AMGX_GS_F32_WIDE");
    k.no_ep_nt = on("AMGX_NO_EP_NT");
    k.no_ep_hoist = on("AMGX_NO_EP_HOIST");
    k.no_dense_tail = on("AMGX_NO_DENSE_TAIL");
    if (const char* e = std::getenv("AMGX_DENSE_MAX")) k.dense_max = std::max<int64_t>(0, std::atoll(e));
    i64("AMGX_COARSE_DENSE_MAX", k.coarse_dense_max);
    k.no_tail_kernel = on("AMGX_NO_TAIL_KERNEL");
    k.no_tail_lds = on("AMGX_NO_TAIL_LDS");
    k.dist_events = on("AMGX_DIST_EVENTS");
    if (const char* e = std::getenv("AMGX_DIST_GRAPH")) k.dist_graph = std::atoi(e) != 0;
    k.dist_no_overlap = on("AMGX_DIST_NO_OVERLAP");
    if (const char* e = std::getenv("AMGX_DIST_FORCE_ALLGATHER")) k.dist_force_allgather = std::string(e) == "pad" ? 2 : 1;
    k.dist_tail_graph = on("AMGX_DIST_TAIL_GRAPH");
    return k;
  }

  // ---- rules that need nothing but the switches (each exists once; the callers add what differs between them)

  // the chunk-local restriction of the fused down kernels: scalar P, 32-bit entry count, not disabled; images with several lanes
  // per row have a switch of their own
  bool fused_restrict_ok(const amgx_matrix& P, int lanes) const {
    return P.br == 1 && P.bc == 1 && P.rowptr[P.n_rows] < I32_MAX && !no_fused_restrict && !(lanes > 1 && no_fused_restrict_multi);
  }
  // local-window images: levels of at least lw_min_rows rows (the callers add their own row-length and shape conditions)
  bool lw_wanted(int64_t rows) const { return rows >= lw_min_rows && !no_lw; }
  bool qlw_wanted(int64_t rows) const { return lw_wanted(rows) && !no_qlw; }
  // window capacity under AMGX_LW_TEST_CAP: of the 512-row chunks of A' and the Gauss-Seidel rest ...
  int64_t lw_cap(int64_t base) const { return lw_test_cap_on ? std::min<int64_t>(base, lw_test_cap) : base; }
  // ... and of the smaller windows of Q and of the block-hybrid sweep (a quarter of it, at least 8)
  int64_t lw_cap_small(int64_t base) const { return lw_test_cap_on ? std::min<int64_t>(base, std::max<int64_t>(8, lw_test_cap / 4)) : base; }
  // compact chunks (cluster_slices) on levels of at least compact_chunks_min_rows rows; see build_restrict_chunks
  bool compact_chunks_wanted(int64_t rows) const { return rows >= compact_chunks_min_rows && !no_compact_chunks; }
};

}  // namespace amgx
