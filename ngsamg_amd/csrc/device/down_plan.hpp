// The shape of a level's fused down launch (pre-smoothing or residual + chunk-local restriction), decided once at create time:
// DownPlan, the value lists of the five kernel templates, and the chunk arithmetic.  resolve_paths (amgx.hip) fills the plans and
// checks them, Handle::down_launch launches from them, amgx_level_paths and amgx_time_op report from them, and the builders
// (build_level.hpp; gs_images.hpp, build_gsb_images) ask the same lists whether a kernel exists.  Host-only: no HIP in here, so a
// plain C++17 compiler builds it (tests/test_down_plan_cpu.py).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include "launch.hpp"          // IntList, contains

namespace amgx {

// Part of the rows a launch covers.  Rank-partitioned levels order their owned rows [interior | boundary] (interior = no ghost
// column; the analogue of the reference's split_ind stages, gssmoother.cpp:664-678): the interior part runs while the halo
// exchange is in flight, the boundary part after it (hybrid_base_smoother.cpp:501-574).
enum { PART_ALL = 0, PART_INT = 1, PART_BND = 2 };
struct Span { int part = PART_ALL; int64_t n_int = 0; };
// A kernel works in units of u rows (slice / window / chunk): the units [a, b) of n_units that the part covers.  Units that
// straddle n_int belong to the boundary part.
inline void unit_range(const Span& sp, int64_t u, int64_t n_units, int64_t& a, int64_t& b) {
  const int64_t split = std::min<int64_t>(n_units, sp.n_int / u);
  if (sp.part == PART_ALL) { a = 0; b = n_units; }
  else if (sp.part == PART_INT) { a = 0; b = split; }
  else { a = split; b = n_units; }
}

// ---- the kernels that exist.  Row-product families: sell_pre_restrict_kernel, sell_win_pre_restrict_kernel,
// sell_lw_pre_restrict_kernel, dia_pre_restrict_kernel, dia_box_pre_restrict_kernel (kernels.hpp)
enum DownFamily : int { DOWN_FAM_SELL = 0, DOWN_FAM_WIN = 1, DOWN_FAM_LW = 2, DOWN_FAM_DIA = 3, DOWN_FAM_DIA_BOX = 4 };
constexpr int DOWN_SLICE = 64;          // lanes of a SELL slice (= WAVE)
constexpr int DOWN_THREADS = 512;       // workgroup size of every form but the one-lane MODE 0 sell form, which has DownSizes
constexpr int DOWN_MULTI_EPT = 4;       // the multi-lane sell form is built for this EPT alone
using DownEpt = IntList<4, 6>;                    // entries of P per thread: sell (one lane per row), win, dia
using DownLwEpt = IntList<2, 4>;                  // ... lw
using DownLwLanes = IntList<2, 4>;                // lanes per row: lw (the builders try them in this order)
using DownSellLanes = IntList<2, 4, 8>;           // ... the multi-lane sell form (one lane per row is a form of its own)
using DownSizes = IntList<256, 512, 1024>;        // workgroup sizes of the one-lane MODE 0 sell form
using DiaDiags = IntList<1, 2, 3, 4, 5, 6, 7, 8>; // upper diagonals: dia
using DiaBoxDiags = IntList<2, 3, 4, 5, 6, 7>;    // ... dia-box
// lanes per row of an image the sell family serves at all
constexpr bool down_sell_lanes_ok(int lanes) { return lanes == 1 || contains(DownSellLanes{}, lanes); }

// ---- the plan.  Values only: std::vector<DevLevel> moves its elements, so the launcher finds the image from (mode, family)
struct DownPlan {
  bool on = false;                      // the level has this fused launch
  // family: a DownFamily; mode: 0 Jacobi from zero, 1 c .* x - A_rest x (after a block-hybrid sweep), 2 rhs - A x (after Chebyshev)
  int family = DOWN_FAM_SELL, mode = 0;
  int threads = 0, lanes = 1, ept = 0;  // workgroup size, lanes per row, entries of P per thread
  int diags = 0, n_chunks = 0;          // upper diagonals (dia, dia-box); chunks = workgroups of the whole level
  int64_t unit_rows = 0;                // rows of a chunk = the unit of the interior / boundary split
  // splittable: consecutive chunks of a sell / win / lw image, otherwise the launch covers the whole level; f32: MODE 2 reads the
  // single-precision image
  bool splittable = false, f32 = false;
  size_t lds_bytes = 0;                 // dynamic LDS (dia-box)
  int64_t box_rows = 0, max_entries = 0; // dia-box: rows of a full box, most entries of P in one box (what the LDS of the NV form holds)
  int lw_max_list = 0;                  // lw: the longest column list of the level's chunks (<= LW_CAP; what the LDS window of the NV form holds)
};

// ---- the same launch on NV = 2 or 4 interleaved vectors (AMGX_MULTI_FUSE_DOWN, DESIGN.md 5.18: sell_pre_restrict_nv_kernel,
// sell_win_pre_restrict_nv_kernel in multi_kernels.hpp).  Built for 512-lane workgroups only: the sell family in the three modes
// (one lane per row with EPT 4 / 6; 2 / 4 / 8 lanes with EPT 4, MODE 0 / 2) and the windowed family in MODE 1.  Every other plan
// keeps the literal stages of the multi-vector cycle.
using DownNvWidths = IntList<2, 4>;
constexpr size_t DOWN_NV_LDS_MAX = 65536;           // static LDS of a workgroup
// static LDS of the NV launch: r of the chunk's rows for NV columns + ONE array of products that the columns use in turn
constexpr size_t down_nv_lds_bytes(const DownPlan& p, int nv) {
  return sizeof(double) * ((size_t)(p.lanes > 0 ? p.threads / p.lanes : 0) * (size_t)nv + (size_t)p.ept * (size_t)p.threads);
}
constexpr bool down_nv_ok(const DownPlan& p, int nv) {
  if (!p.on || !contains(DownNvWidths{}, nv) || p.threads != DOWN_THREADS) return false;
  bool shape = false;
  if (p.family == DOWN_FAM_SELL && p.mode >= 0 && p.mode <= 2)
    shape = p.lanes == 1 ? contains(DownEpt{}, p.ept) : (p.mode != 1 && contains(DownSellLanes{}, p.lanes) && p.ept == DOWN_MULTI_EPT);
  else if (p.family == DOWN_FAM_WIN)
    shape = p.mode == 1 && p.lanes == 1 && contains(DownEpt{}, p.ept);
  return shape && down_nv_lds_bytes(p, nv) <= DOWN_NV_LDS_MAX;
}

// ---- the diagonal-image launches on NV = 2 or 4 interleaved vectors (AMGX_MULTI_FUSE_DOWN_DIA, DESIGN.md 5.19:
// dia_pre_restrict_nv_kernel, dia_box_pre_restrict_nv_kernel in multi_kernels.hpp).  A rule of its own beside down_nv_ok, which keeps
// refusing both families: the capability has its own opt-in bit.
// LDS of the launch.  512-row chunks: r of the chunk's rows for NV columns + ONE array of products that the columns use in turn
// (ChunkRestrictNV), static.  Box chunks: r of the box for NV columns, then the published x_j for NV columns, which the products of
// ONE column at a time replace; dynamic.
constexpr size_t DOWN_NV_DIA_LDS_MAX = 163840;      // the 160 KiB of LDS a workgroup may declare on gfx950
constexpr size_t down_nv_dia_lds_bytes(const DownPlan& p, int nv) {
  if (p.family == DOWN_FAM_DIA) return sizeof(double) * ((size_t)DOWN_THREADS * (size_t)nv + (size_t)p.ept * (size_t)DOWN_THREADS);
  if (p.family != DOWN_FAM_DIA_BOX) return 0;
  if (p.box_rows < 0 || p.max_entries < 0) return ~(size_t)0;  // (never a plan of resolve_paths: refused by the bound)
  const size_t xs = (size_t)p.box_rows * (size_t)nv;
  return sizeof(double) * (xs + std::max(xs, (size_t)p.max_entries));
}
// The LDS bound is a guard, not a filter: a box has at most 2048 rows (dia::BOX_MAX_ROWS) and its entries fit 10240 - box_rows
// doubles (DIA_BOX_LDS_DOUBLES, the single-vector kernel's LDS), so the fullest box a level can have needs
// 8 * (4 * 2048 + max(4 * 2048, 8192)) = 128 KiB at NV = 4; the 512-row form needs 40 KiB at most.
constexpr bool down_nv_dia_ok(const DownPlan& p, int nv) {
  if (!p.on || !contains(DownNvWidths{}, nv) || p.mode != 0 || p.threads != DOWN_THREADS || p.lanes != 1) return false;
  bool shape = false;
  if (p.family == DOWN_FAM_DIA) shape = contains(DiaDiags{}, p.diags) && contains(DownEpt{}, p.ept);
  else if (p.family == DOWN_FAM_DIA_BOX) shape = contains(DiaBoxDiags{}, p.diags);
  return shape && down_nv_dia_lds_bytes(p, nv) <= DOWN_NV_DIA_LDS_MAX;
}

// ---- the local-window launch on NV = 2 or 4 interleaved vectors (AMGX_MULTI_FUSE_DOWN_F32, DESIGN.md 5.23:
// sell_lw_pre_restrict_nv_kernel in multi_kernels.hpp).  A rule of its own beside down_nv_ok, which keeps refusing the family: the
// capability has its own opt-in bit.  Built for MODE 1 alone (the residual after a block-hybrid sweep from zero on the local-window
// image of `rest`), 512 lanes per workgroup, the lanes and EPT of the single-vector family.
// LDS of the launch, dynamic: the window x[ccol[k]] of the longest list for NV columns, r of the chunk's rows for NV columns, ONE
// array of products that the columns use in turn (ChunkRestrictNV).  The bound is the 160 KiB of DOWN_NV_DIA_LDS_MAX.
constexpr size_t down_nv_lw_lds_bytes(const DownPlan& p, int nv) {
  if (p.lanes <= 0 || p.lw_max_list < 0 || p.ept < 0 || nv < 0) return ~(size_t)0;     // (never a plan of resolve_paths: refused by the bound)
  return sizeof(double) * ((size_t)p.lw_max_list * (size_t)nv + (size_t)(DOWN_THREADS / p.lanes) * (size_t)nv + (size_t)p.ept * (size_t)DOWN_THREADS);
}
constexpr bool down_nv_lw_ok(const DownPlan& p, int nv) {
  if (!p.on || !contains(DownNvWidths{}, nv) || p.family != DOWN_FAM_LW || p.mode != 1 || p.threads != DOWN_THREADS) return false;
  if (!contains(DownLwLanes{}, p.lanes) || !contains(DownLwEpt{}, p.ept)) return false;
  return down_nv_lw_lds_bytes(p, nv) <= DOWN_NV_DIA_LDS_MAX;
}

// ---- chunk arithmetic.  A chunk is what one workgroup of `threads` lanes owns: threads / 64 slices = threads / lanes rows
constexpr int down_slices_per_chunk(int threads) { return threads / DOWN_SLICE; }
constexpr int64_t down_rows_per_chunk(int threads, int lanes) { return threads / lanes; }
// chunks of consecutive slices.  n: sell / win / lw: the slices of the image (64 lanes each, i.e. 64 / lanes rows); dia: the
// rows of the level; dia-box: the boxes, one chunk each
constexpr int64_t down_expected_chunks(int family, int64_t n, int threads, int lanes) {
  const int64_t slices = family == DOWN_FAM_DIA ? (n * lanes + DOWN_SLICE - 1) / DOWN_SLICE : n, spc = down_slices_per_chunk(threads);
  return family == DOWN_FAM_DIA_BOX ? n : (slices + spc - 1) / spc;
}
// only ranges of consecutive chunks can be split; the diagonal-image forms run the whole level in one launch
constexpr bool down_splittable(int family, bool compact) { return !compact && (family == DOWN_FAM_SELL || family == DOWN_FAM_WIN || family == DOWN_FAM_LW); }
// the chunks [a, b) a launch over `sp` covers; false: the plan refuses the part (an unsplittable launch asked for less than all)
inline bool down_chunk_range(const DownPlan& p, const Span& sp, int64_t& a, int64_t& b) {
  if (!p.splittable && sp.part != PART_ALL) return false;
  unit_range(sp, p.unit_rows, p.n_chunks, a, b);
  return true;
}

}  // namespace amgx
