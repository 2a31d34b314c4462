// Which handles run fused column groups in the multi-vector calls: the rule, stated once.
// multi.hpp fills a MultiLevelFacts per level from the handle and asks multi_handle_rule once per rule; a call's flags then pick
// the rule in force (multi_rule_in_force) and whether it runs fused groups (multi_runs_fused).  A new refusal is ONE line in
// multi_level_reason (and a fact in MultiLevelFacts where it reads something new).  Host-only: no HIP and no Handle in here, so a
// plain C++17 compiler builds it (tests/test_multi_rule_cpu.py compares it with the four rules written out separately).
#pragma once
#include <cstdint>
#include <string>
#include "../../../include/amgx.h"      // AMGX_SM_*, AMGX_MULTI_FUSE*

namespace amgx {

// greedy cut of k columns into fused widths 4, 2 plus at most one single column.  The kernels are written for any NV, but width 8
// is not instantiated: sell_spmm_kernel<G, 8, EP> needs 134-144 VGPRs = 3 waves per SIMD (66 / 90-98 VGPRs, 7 / 4-5 waves at
// widths 2 / 4), and measured at cfg 2 its level-0 passes cost 183 us per column against 145 us at width 4, the
// whole cycle 1.23 x k single applications against 1.40 x -- so 8 columns run as 4 + 4
inline int multi_groups(int k, bool fused, int32_t* width) {
  int n = 0;
  if (!fused) { for (int j = 0; j < k; ++j) width[n++] = 1; return n; }
  for (int w : {4, 2, 1})
    while (k >= w) { width[n++] = w; k -= w; }
  return n;
}

// what the rule reads of one level
struct MultiLevelFacts {
  int bs = 1;
  bool empty = false;                   // n == 0: nothing is launched, so the formats are not asked
  bool square = true;                   // n == ncols (no ghost columns)
  bool permuted = false;                // stored in another numbering than the caller's
  bool jacobi_f32 = false;              // single-precision Jacobi images; the NV kernels read fp64 images
  bool gs_f32 = false;                  // single-precision Gauss-Seidel images
  bool sgs_f32 = false;                 // ... of a scalar level (the twin too): the fp64 values of its sweep images are released
  // the call carries AMGX_MULTI_FUSE_F32 and every image this level's fused passes read has a multi-vector kernel on its float array
  // (Handle::multi_f32_ok)
  bool f32_ok = false;
  bool smoothed = false;                // not the coarsest level
  int sm_type = AMGX_SM_JACOBI;
  bool plain = true;                    // sm_steps == 1 and no sm_symm
  int cheb_degree = 0;
  // which matrices have a kernel on NV vectors (Handle::multi_*_ok, next to the launchers)
  bool a_scalar = false;                // multi_scalar_ok(A)
  bool a_level = false;                 // multi_level_ok(A) with blocks of the level's size
  bool t_scalar = false;                // multi_scalar_ok of P and of P^T
  bool t_transfer = false;              // multi_transfer_ok of P and of P^T
  bool sweep_ok = false;                // multi_sweep_ok
  bool block_sweep_ok = false;          // multi_block_sweep_ok
  bool block_sweep_fits = false;        // multi_block_sweep_fits
};

// The first reason the level keeps the column loop under `rule` (0: no flag; 1: AMGX_MULTI_FUSE; 2: ..._GS; 3: ..._GS_BLOCK), or
// nullptr.  The order of the questions is part of the interface (amgx_multi_note returns the first reason): rule 0 asks the
// level first and then the smoother, the wider rules the smoother first (it is the reason a caller can act on).
inline const char* multi_level_reason(int rule, const MultiLevelFacts& f) {
  const bool base = rule == 0;
  const bool jacobi = f.sm_type == AMGX_SM_JACOBI, cheby = f.sm_type == AMGX_SM_CHEBY;
  const bool gs = f.smoothed && rule >= 2 && f.sm_type == AMGX_SM_GS;       // rule >= 2 admits AMGX_SM_GS
  auto smoother = [&]() -> const char* {
    if (!f.smoothed) return nullptr;
    if (rule >= 2 && f.sm_type == AMGX_SM_BGS) return "block Gauss-Seidel (bgs) smoother";
    if (rule == 2 && gs && f.bs != 1) return "Gauss-Seidel on a block level";       // (rule 3 asks the level's sweep form below)
    if (!(jacobi || (cheby && !base) || gs))
      return base ? "smoother is not Jacobi" : rule == 1 ? "smoother is not Jacobi or Chebyshev" : "smoother is not Jacobi, Chebyshev or Gauss-Seidel";
    if (!f.plain) return "sm_steps > 1 or sm_symm";
    if (cheby && (f.cheb_degree < 1 || f.cheb_degree > 8)) return "Chebyshev level without coefficients";
    return nullptr;
  };
  auto level = [&]() -> const char* {
    if (base && f.bs != 1) return "block level";
    if (f.bs != 1 && f.bs != 2 && f.bs != 3 && f.bs != 6) return "block size is not 1, 2, 3 or 6";
    if (!f.square) return "ghost columns";
    if (f.permuted) return "renumbered level";
    if (f.jacobi_f32) return "single-precision Jacobi images";
    if (gs && !f.empty) {
      // (without AMGX_MULTI_FUSE_F32 the fused sweeps read fp64 images: the column loop keeps a column equal to amgx_apply, bit for
      // bit.  With it, f32_ok says that the fused passes read the arrays of the single-vector passes)
      if (rule >= 3 && f.gs_f32 && !f.f32_ok) return "single-precision Gauss-Seidel images";
      if (f.sgs_f32 && !f.f32_ok) return "single-precision Gauss-Seidel images";
      if (!(f.bs == 1 ? f.sweep_ok : f.block_sweep_ok)) return "Gauss-Seidel sweep form without a multi-vector kernel";
      if (f.bs != 1 && !f.block_sweep_fits) return "sweep block too large for the multi-vector sweep";
    }
    if (!f.empty && !(base ? f.a_scalar : f.a_level)) return "level matrix format";
    return nullptr;
  };
  const char* why = base ? level() : smoother();
  if (!why) why = base ? smoother() : level();
  if (!why && f.smoothed && !f.empty && !(base ? f.t_scalar : f.t_transfer)) why = "transfer format";
  return why;
}

// all or nothing per handle: a V cycle whose levels all pass.  why: "" on a fused handle, else the first reason with its level
struct MultiDecision { int fused = 0; std::string why; };
inline MultiDecision multi_handle_rule(int rule, bool cycle_is_v, const MultiLevelFacts* lev, int n_levels) {
  if (!cycle_is_v) return {0, "cycle is not V"};
  for (int l = 0; l < n_levels; ++l)
    if (const char* why = multi_level_reason(rule, lev[l])) return {0, std::string(why) + " (level " + std::to_string(l) + ")"};
  return {1, ""};
}

// ---- a call's flags.  AMGX_MULTI_FUSE_GS_BLOCK implies ..._GS implies AMGX_MULTI_FUSE; the two ..._DOWN bits imply nothing here.
// AMGX_MULTI_FUSE_F32 implies nothing either: it picks which of the two decisions per rule is read (the facts with f32_ok filled in).
// fused[r]: the handle under rule r (each rule admits what the one before admits).
constexpr int MULTI_RULE_FLAGS = AMGX_MULTI_FUSE | AMGX_MULTI_FUSE_GS | AMGX_MULTI_FUSE_GS_BLOCK;
inline int multi_asked_rule(int flags) {        // the widest rule the flags ask for
  return flags & AMGX_MULTI_FUSE_GS_BLOCK ? 3 : flags & AMGX_MULTI_FUSE_GS ? 2 : flags & AMGX_MULTI_FUSE ? 1 : 0;
}
// the rule in force: the flags decide the path only where the narrower rule does not hold (a scalar Jacobi handle: one path, one
// graph; a handle without Gauss-Seidel levels runs the same cycle under all flags, one without block Gauss-Seidel levels the
// same cycle under the two Gauss-Seidel flags).  So: the narrowest rule that admits the handle, else the widest one asked for.
inline int multi_rule_in_force(int flags, const int* fused) {
  const int asked = multi_asked_rule(flags);
  for (int r = 0; r < asked; ++r) if (fused[r] == 1) return r;
  return asked;
}
inline bool multi_runs_fused(int flags, const int* fused) {
  for (int r = 0; r <= multi_asked_rule(flags); ++r) if (fused[r] == 1) return true;
  return false;
}

}  // namespace amgx
