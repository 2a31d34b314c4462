// Multi-vector apply path: k right-hand sides per matrix pass.
//
// Reference interface: BaseMatrix::Mult on an NGSolve MultiVector (what LOBPCG / PINVIT and callers with several load cases
// hand to a preconditioner); the reference runs AMGMatrix::Mult once per vector.  Here a handle whose smoothed levels are all
// scalar, plain Jacobi levels of a V-cycle runs the LITERAL cycle (x = w Dinv b, r = b - A x, b_c = P^T r, ..., t = x + P x_c,
// x = t + w Dinv (b - A t): amg_matrix.cpp:183-302) on the level images A, P, P^T with every matrix entry read ONCE for NV = 2 or 4
// vectors.  Inside the handle multi-vectors are interleaved, entry (row i, column j) at i*NV + j: a gathered column index
// then costs one address and 8*NV contiguous bytes.  Every other handle answers the same calls through a column loop over the
// single-vector path -- unless the call carries AMGX_MULTI_FUSE: then handles whose smoothed levels are plain
// Jacobi or Chebyshev levels with block size 1, 2, 3 or 6 run fused groups too.  AMGX_MULTI_FUSE_GS implies that
// flag and admits scalar Gauss-Seidel levels in the block-hybrid or the multicolour form as well.  AMGX_MULTI_FUSE_GS_BLOCK (DESIGN.md
// 5.16) implies both and admits Gauss-Seidel on 2x2 / 3x3 / 6x6 levels in the hybrid-block, block-coloured and the two block multicolour
// forms.  The Gauss-Seidel step on NV vectors is the single-vector one: Handle::sweep<NV>, sweep_from_zero<NV> and
// residual_after_zero<NV> (amgx.hip) route it, Handle::gs_sweep<NV>, gsb_sweep<NV> and bgsb_sweep<NV> launch it; this file adds the
// width dispatch (Multi::width) and nothing else.
//
// This file is the host side.  The four rules are ONE function, multi_level_reason (multi_rule.hpp, host-only), on
// the facts that Multi::facts reads from a level; the cut of k columns into groups, the packing of the caller's columns and the
// single-column fallback are ONE walker, Multi::walk, and what the C entry points do around their one call is multi_call.  The
// kernels are in multi_kernels.hpp; which of them serves a matrix is decided in ONE place, Handle::product<NV, EP> (amgx.hip),
// next to the value lists that Handle::multi_*_ok ask; the Chebyshev recurrence is cheb_schedule (cheb_schedule.hpp), the one
// Handle::cheb_smooth runs.
#pragma once
#include "multi_rule.hpp"      // multi_groups, MultiLevelFacts, multi_level_reason, multi_handle_rule, the flag logic

namespace amgx {

struct MultiWork {                      // work vectors of one fused width, kept from call to call
  // d: the update vector of a Chebyshev level; part: the partial sums of the fused down pass (AMGX_MULTI_FUSE_DOWN, n_slots * width)
  struct Lev { DevBuf<double> x, rhs, res, tmp, d, part; };
  std::vector<Lev> lev;
  DevBuf<double> in, out;               // interleaved copies of a group of the caller's columns (arguments that are not used in place)
};

struct MultiState {
  // the handle under rule 0 (no flag), 1 (AMGX_MULTI_FUSE), 2 (..._GS: plus scalar Gauss-Seidel levels, 5.15) and
  // 3 (..._GS_BLOCK: plus Gauss-Seidel on square-block levels, 5.16).  -1: not decided yet; 0: why[.][r] is the first reason.
  // First index: the call carries AMGX_MULTI_FUSE_F32 (5.22), which fills MultiLevelFacts::f32_ok and the two sweep answers in.
  int fused[2][4] = {{-1, -1, -1, -1}, {-1, -1, -1, -1}};
  std::string why[2][4];
  std::vector<MultiLevelFacts> facts[2]; // what the rules read, per level
  MultiWork work[MULTI_MAX + 1];        // by width (2, 4)
  DevBuf<double> col_in, col_out;       // one contiguous column (single-vector path behind an interleaved argument)
  DevBuf<double> stage_b, stage_x, stage_c;   // host-pointer calls (stage_c: the coarse multi-vector of amgx_down_multi)
  DevBuf<double> dn_c, dn_d, dn_part, dn_col; // amgx_down_multi: interleaved b_c, Chebyshev update and partial sums of a group; b_c of a single column
  DevBuf<double> sm_x, sm_b, sm_t, sm_r; // amgx_smooth_multi: interleaved x, b and the sweep's other buffer of a group; res of a single column
  DevBuf<double> kr[5];                 // amgx_pcg_multi: b, x, d, w, s (interleaved, width k)
  DevBuf<double> kr_sc, kr_partial;
  DevBuf<int32_t> kr_active;
  // b, x, k, layout, ldb, ldx, rule in force (0 .. 3; + 4: fused down passes, AMGX_MULTI_FUSE_DOWN on a handle with a level that takes one;
  // + 8: AMGX_MULTI_FUSE_DOWN_DIA on a handle where it changes a level's form or fold; + 16: AMGX_MULTI_FUSE_F32 on a handle where it
  // changes the decision; + 32: AMGX_MULTI_FUSE_DOWN_F32 on a handle where it changes a level's form)
  using Key = std::tuple<const double*, double*, int, int, int64_t, int64_t, int>;
  GraphCache<Key> graphs;
};

void multi_drop_graphs(MultiState* s) { s->graphs.drop(); }       // amgx_set_stream: captures of the old stream go
void multi_free(MultiState* s) { delete s; }

// a caller's multi-vector on the device: entry (row i, column j) at p[i * rs + j * cs]
struct MultiView {
  double* p = nullptr;
  int64_t rs = 1, cs = 0;
  MultiView() = default;
  MultiView(const double* q, int k, int64_t ld, bool interleaved) : p(const_cast<double*>(q)), rs(interleaved ? k : 1), cs(interleaved ? 1 : ld) {}
};
// one argument of a walk over column groups (Multi::walk).  A single column of an interleaved argument is packed into `col`
// (col_len doubles); a fused group into `grp` (rows * MULTI_MAX / 2 doubles: the widest group), or with grp == nullptr into the
// in / out copy of the width's work space -- unless the argument is exactly that group already, which is then used in place.
enum { MULTI_ARG_IN = 1, MULTI_ARG_OUT = 2 };
struct MultiArg { int role; MultiView v; int64_t rows; DevBuf<double>* col; int64_t col_len; DevBuf<double>* grp; };

struct Multi {
  Handle& h;
  MultiState& st;
  static constexpr int ALL_FLAGS = MULTI_RULE_FLAGS;                                                   // the flags that widen the rule
  static constexpr int DOWN_FLAGS = AMGX_MULTI_FUSE_DOWN | AMGX_MULTI_FUSE_DOWN_DIA | AMGX_MULTI_FUSE_DOWN_F32;   // (the second implies the first, nothing else)
  static constexpr int CALL_FLAGS = ALL_FLAGS | DOWN_FLAGS | AMGX_MULTI_FUSE_F32;                     // ... and the ones that imply nothing about the rule
  static constexpr int NOTE_FLAGS = ALL_FLAGS | AMGX_MULTI_FUSE_F32 | AMGX_MULTI_FUSE_DOWN_F32;       // what amgx_multi_note looks at
  // AMGX_MULTI_FUSE_DOWN_F32 implies AMGX_MULTI_FUSE_DOWN and AMGX_MULTI_FUSE_F32 and nothing else
  static constexpr int implied(int fl) { return fl & AMGX_MULTI_FUSE_DOWN_F32 ? fl | AMGX_MULTI_FUSE_DOWN | AMGX_MULTI_FUSE_F32 : fl; }
  const int flags;
  const int fb;                         // the call carries AMGX_MULTI_FUSE_F32: which decision of MultiState is read
  const bool block_flag;                // the call carries AMGX_MULTI_FUSE_GS_BLOCK (which implies the flag below)
  const bool gs_flag;                   // the call carries AMGX_MULTI_FUSE_GS (which implies AMGX_MULTI_FUSE)
  const bool fz;                        // this call runs fused groups
  const bool down_flag;                 // the call carries AMGX_MULTI_FUSE_DOWN: modifies the fused groups, implies nothing
  const bool dia_flag;                  // the call carries AMGX_MULTI_FUSE_DOWN_DIA: implies down_flag; diagonal-image levels take the pass too
  const bool d32_flag;                  // the call carries AMGX_MULTI_FUSE_DOWN_F32: implies down_flag and fb; levels with float Gauss-Seidel images take the pass too
  explicit Multi(Handle& hh, int fl = 0)
      : h(hh), st(state(hh)), flags(implied(fl)), fb(flags & AMGX_MULTI_FUSE_F32 ? 1 : 0), block_flag(fl & AMGX_MULTI_FUSE_GS_BLOCK), gs_flag(multi_asked_rule(fl) >= 2),
        fz(multi_runs_fused(flags, st.fused[fb])), down_flag(fl & DOWN_FLAGS), dia_flag(fl & AMGX_MULTI_FUSE_DOWN_DIA), d32_flag(fl & AMGX_MULTI_FUSE_DOWN_F32) {
    if (down_flag) for (int l = 0; l < h.n_levels(); ++l) dn.push_back(level_down(l, dia_flag, d32_flag));     // once per call
  }
  int rule() const { return multi_rule_in_force(flags, st.fused[fb]); }   // (part of the graph key)
  const std::string& note() const { return st.why[fb][rule()]; }
  // AMGX_MULTI_FUSE_F32 changes what this call runs (part of the graph key on such handles only, like dia_active)
  bool f32_active() const { return fb && (fz != multi_runs_fused(flags, st.fused[0]) || rule() != multi_rule_in_force(flags, st.fused[0])); }

  // what the rule reads of a level: the only place that asks Handle::multi_*_ok
  static MultiLevelFacts facts(const Handle& h, int l, bool f32) {
    const DevLevel& V = h.lev[l];
    MultiLevelFacts f;
    f.bs = V.bs; f.empty = V.n == 0; f.square = V.n == V.ncols; f.permuted = h.permuted(l);
    f.jacobi_f32 = V.jp32 || V.jp32_wide; f.gs_f32 = V.gs32 || V.gs32_wide; f.sgs_f32 = V.sgs32 || V.sgs32_wide;
    f.smoothed = l + 1 < h.n_levels(); f.sm_type = V.sm_type; f.plain = h.plain(V); f.cheb_degree = V.cheb_degree;
    f.a_scalar = Handle::multi_scalar_ok(V.A); f.a_level = Handle::multi_level_ok(V.A) && V.A.br == V.bs;
    f.t_scalar = Handle::multi_scalar_ok(V.P) && Handle::multi_scalar_ok(V.PT);
    f.t_transfer = Handle::multi_transfer_ok(V.P) && Handle::multi_transfer_ok(V.PT);
    f.sweep_ok = h.multi_sweep_ok(V, f32); f.block_sweep_ok = h.multi_block_sweep_ok(V, f32); f.block_sweep_fits = h.multi_block_sweep_fits(V);
    f.f32_ok = f32 && h.multi_f32_ok(V);
    return f;
  }
  static MultiState& state(Handle& h) {
    if (!h.multi) h.multi = new MultiState;
    MultiState& s = *h.multi;
    if (s.fused[0][0] < 0) {
      for (int b = 0; b < 2; ++b) {
        for (int l = 0; l < h.n_levels(); ++l) s.facts[b].push_back(facts(h, l, b == 1));
        for (int r = 0; r < 4; ++r) {
          MultiDecision d = multi_handle_rule(r, h.cycle == AMGX_CYCLE_V, s.facts[b].data(), h.n_levels());
          s.fused[b][r] = d.fused; s.why[b][r] = std::move(d.why);
        }
      }
    }
    return s;
  }
  // first level that the multi cycle hands to ONE dense product (collapsed operator or the coarsest level's inverse)
  // (0: the whole cycle is the dense operator, no level work vectors)
  int top() const { return h.dense_level >= 0 ? h.dense_level : tail_cols() ? h.tail_level : h.n_levels() - 1; }
  // AMGX_MULTI_FUSE_F32 on a handle with single-precision Gauss-Seidel images (`exact`): where the single-vector
  // cycle of a Gauss-Seidel level differs from the literal stages, the fused group takes the single-vector kernel per column, so that a
  // column reads the values and keeps the order of additions of amgx_apply.  tail_cols: the levels from tail_level on run as the
  // single-workgroup tail program (which reads its own fp64 copies of the TRUE A, never the float images).  col_down: the residual
  // after the sweep from zero runs fused with the chunk-local restriction (DOWN_GSB), which has no multi-vector form on float images.
  bool exact() const {
    if (!fb) return false;
    for (const DevLevel& V : h.lev) if (V.sgs32 || V.sgs32_wide || V.gs32 || V.gs32_wide) return true;
    return false;
  }
  bool tail_cols() const { return h.dense_level < 0 && h.tail_level > 0 && exact(); }
  bool col_down(int l) const { const DevLevel& V = h.lev[l]; return V.sm_type == AMGX_SM_GS && V.paths.down == DOWN_GSB && !level_down(l).form && exact(); }
  // col_block: a Gauss-Seidel level with square blocks.  On one vector Handle::product picks the kernel of a block-CSR matrix per matrix
  // (row-lane or vector form), on NV vectors there is one kernel with another order of additions; so the transfers P^T and P and the
  // coarsest solve run per column.  The sweeps are fused, and so is the residual after the sweep from zero where it reads a BSELL image
  // (res_fused: `rest` / `bupper` of a level with the split, else A in BSELL): the NV BSELL kernels keep the single-vector order.
  bool col_block(int l) const { const DevLevel& V = h.lev[l]; return V.sm_type == AMGX_SM_GS && V.bs != 1 && exact(); }
  bool res_fused(int l) const {
    const DevLevel& V = h.lev[l];
    if (!Handle::split_identity(V, 2)) return V.A.fmt == FMT_BSELL;
    return !V.paths.bgsb() || V.bgsb.rest.fmt == FMT_BSELL;
  }
  bool col_coarse() const { return h.lev.back().bs != 1 && exact(); }
  bool col_stages() const {
    if (tail_cols() || col_coarse()) return true;
    for (int l = 0; l < top(); ++l) if (col_down(l) || col_block(l)) return true;
    return false;
  }
  // the contiguous column buffers of those stages (allocated before a capture)
  void fit_cols() {
    const int64_t n0 = h.lev[0].len();
    fit(st.col_in, n0); fit(st.col_out, n0); fit(st.dn_col, n0); fit(st.sm_r, n0);
  }

  // ---- AMGX_MULTI_FUSE_DOWN: the down pass of ONE smoothed level on a fused group.  form 0: the literal stages,
  // `why` says which property keeps them ("" without the bit, on an empty level and on a level that is not smoothed); form 1 / 2:
  // Handle::down_launch_nv on `plan` (sell / windowed sell).  fold: a Jacobi level whose way up is x = z + Q x_c.  The rule is
  // down_nv_ok (down_plan.hpp) on the plan the single-vector cycle runs for the level's smoother.
  // AMGX_MULTI_FUSE_DOWN_DIA (`dia`): form 3 / 4: the same launch on a diagonal-image plan with 512-row / box chunks
  // (rule: down_nv_dia_ok), and a Jacobi level that takes a fused down pass folds the way up through the plain windowed Q even where
  // the single-vector cycle runs the local-window image QLW of it.  Without that bit both stay as AMGX_MULTI_FUSE_DOWN alone has them.
  struct DownNv { int form = 0, mode = 0; bool fold = false, f32 = false; const DownPlan* plan = nullptr; const char* why = ""; };
  std::vector<DownNv> dn;               // level_down of every level under this call's flags (empty without AMGX_MULTI_FUSE_DOWN)
  DownNv level_down(int l) const { return l >= 0 && l < (int)dn.size() ? dn[l] : DownNv(); }
  // AMGX_MULTI_FUSE_DOWN_F32 (`d32`): a Gauss-Seidel level with single-precision images whose single-vector cycle runs
  // plan_rg takes the pass too, where Handle::multi_f32_ok holds and the image the launch reads has the array the single-vector launch
  // reads (the float array where the plan says f32, the rounded values at fp64 width on the AMGX_GS_F32_WIDE twin); form 5: the
  // local-window image of `rest` (rule: down_nv_lw_ok), admitted on such levels alone.
  DownNv level_down(int l, bool dia, bool d32) const {
    DownNv d;
    if (!down_flag || l < 0 || l + 1 >= h.n_levels()) return d;
    const MultiLevelFacts& f = st.facts[fb][l]; // (the first two refusals are the fusion rule's, on the same facts)
    if (f.empty) return d;
    const DevLevel& V = h.lev[l];
    if (f.bs != 1) { d.why = "block level"; return d; }
    if (f.jacobi_f32) { d.why = "single-precision Jacobi images"; return d; }     // (the NV kernels read fp64 images)
    if (f.sgs_f32) {                                                              // (... and the fp64 values of `rest` are released)
      // a fused pass reads the array the single-vector pass of the same handle reads: lifted for plan_rg under the bit, nowhere else
      bool lifted = d32 && f.f32_ok && V.sm_type == AMGX_SM_GS && V.paths.sweep == SWEEP_GSB && V.paths.down == DOWN_GSB && V.plan_rg.on && Handle::split_identity(V, 2);
      if (lifted) {
        const DevMatrix& M = down_image(V, 1, V.plan_rg.family == DOWN_FAM_LW);
        lifted = M.fmt == FMT_SELL && (V.plan_rg.f32 ? M.has32() : (V.sgs32_wide && M.sell.val.p != nullptr));
      }
      if (!lifted) { d.why = "single-precision Gauss-Seidel images"; return d; }
    }
    const DownPlan* p = nullptr;
    if (f.square && !f.permuted && !st.facts[fb][l + 1].permuted && f.plain) {
      if (V.sm_type == AMGX_SM_GS) {
        if (V.paths.sweep != SWEEP_GSB) { d.why = "multicolour sweep"; return d; }
        if (V.paths.down == DOWN_GSB && V.plan_rg.on && Handle::split_identity(V, 2)) p = &V.plan_rg;     // (2: any width above one)
      } else if (V.sm_type == AMGX_SM_JACOBI) {
        if (V.paths.jacobi_down() && V.plan_rf.on) p = &V.plan_rf;
      } else if (V.sm_type == AMGX_SM_CHEBY) {
        if (V.paths.down == DOWN_CHEB && V.plan_rf.on) p = &V.plan_rf;
      }
    }
    if (!p) { d.why = "no chunk-local restriction"; return d; }
    d.plan = p;                                                                   // (also of a level that stays literal: amgx_multi_level_plan reports its shape)
    if (p->family == DOWN_FAM_LW) {                                               // (on levels with float Gauss-Seidel images under their bit alone)
      if (!d32 || !f.sgs_f32 || !down_nv_lw_ok(*p, 2) || !down_nv_lw_ok(*p, 4)) { d.why = "local-window image"; return d; }
      d.form = 5; d.mode = p->mode; d.f32 = p->f32; d.plan = p;
      return d;
    }
    if (p->family == DOWN_FAM_DIA || p->family == DOWN_FAM_DIA_BOX) {
      if (!dia || !down_nv_dia_ok(*p, 2) || !down_nv_dia_ok(*p, 4)) { d.why = "diagonal image"; return d; }
      d.form = p->family == DOWN_FAM_DIA ? 3 : 4;
      d.mode = 0; d.plan = p;
      d.fold = h.folded(V) && !V.Q.empty() && Handle::multi_scalar_ok(V.Q);      // (a diagonal image is a Jacobi level's)
      return d;
    }
    if (p->threads != DOWN_THREADS) { d.why = "workgroup size"; return d; }
    // (what is left: the windowed image of A' behind the AMGX_APRE_WINDOW A/B hook, which has no multi-vector kernel)
    if (!down_nv_ok(*p, 2) || !down_nv_ok(*p, 4)) { d.why = "windowed image"; return d; }
    d.form = p->family == DOWN_FAM_SELL ? 1 : 2;
    d.mode = p->mode; d.f32 = p->f32; d.plan = p;
    d.fold = V.sm_type == AMGX_SM_JACOBI && h.folded(V) && !V.Q.empty() && Handle::multi_scalar_ok(V.Q) && (dia || V.QLW.empty());
    return d;
  }
  static int64_t down_slots(const DevLevel& V, const DownNv& d) { return d.form ? (d.mode == 1 ? V.RG : V.RF).n_slots : 0; }
  // the cycle of this call runs at least one fused down pass (part of the graph key)
  bool down_active() const {
    if (!down_flag || !fz) return false;
    for (int l = 0; l < top(); ++l) if (level_down(l).form) return true;
    return false;
  }
  // ... and AMGX_MULTI_FUSE_DOWN_DIA changes the form or the fold of at least one of its levels (part of the key on such handles only)
  bool dia_active() const {
    if (!dia_flag || !fz) return false;
    for (int l = 0; l < top(); ++l) {
      const DownNv a = level_down(l), b = level_down(l, false, d32_flag);
      if (a.form != b.form || a.fold != b.fold) return true;
    }
    return false;
  }
  // ... and AMGX_MULTI_FUSE_DOWN_F32 the form of at least one of its levels (part of the key on such handles only)
  bool d32_active() const {
    if (!d32_flag || !fz) return false;
    for (int l = 0; l < top(); ++l) if (level_down(l).form != level_down(l, dia_flag, false).form) return true;
    return false;
  }
  template <class Ops>
  void down_nv(int w, int l, const DownNv& d, const Ops& o, double* part, double* b_coarse) {
    width(w, [&](auto W) { h.down_launch_nv<W()>(l, *d.plan, o, part, b_coarse); });
  }

  int64_t work_bytes(int k) const {
    if (k == 1) return 0;                                       // amgx_apply itself
    int32_t wd[MULTI_MAX];
    const int ng = multi_groups(k, fz, wd);
    const int64_t n0 = h.lev[0].len();
    const int T = top();
    int64_t per_col = 2 * n0;                                  // the two interleaved copies of a group of the caller's columns
    for (int l = 0; l <= T && l < h.n_levels(); ++l)           // (a Chebyshev level: one more vector, the update d)
      per_col += ((l > 0 ? 2 : 0) + (l < T ? 2 + (h.lev[l].sm_type == AMGX_SM_CHEBY ? 1 : 0) : 0)) * h.lev[l].len();
    if (fz)                                                     // (AMGX_MULTI_FUSE_DOWN: the partial sums of every fused down pass)
      for (int l = 0; l < T && l + 1 < h.n_levels(); ++l) per_col += down_slots(h.lev[l], level_down(l));
    int64_t bytes = 0;
    bool single = false, seen[MULTI_MAX + 1] = {};              // (groups of one width share their work space)
    for (int g = 0; g < ng; ++g) {
      if (wd[g] == 1) single = true;
      else if (!seen[wd[g]]) { seen[wd[g]] = true; bytes += per_col * wd[g] * (int64_t)sizeof(double); }
    }
    if (single) bytes += 2 * n0 * (int64_t)sizeof(double);    // one contiguous column in, one out
    return bytes;
  }

  static void fit(DevBuf<double>& b, int64_t n) { if ((int64_t)b.n < n) b.alloc((size_t)n); }
  MultiWork& work(int w) {
    MultiWork& W = st.work[w];
    if (W.lev.empty()) {                                        // (top() is the same for every fused call of a handle: a handle that
      const int T = top();                                      //  AMGX_MULTI_FUSE_F32 fuses is not fused without it)
      W.lev.resize(T + 1);
      for (int l = 0; l <= T; ++l) {
        const size_t len = (size_t)h.lev[l].len() * w;
        if (l > 0) { W.lev[l].x.alloc(len); W.lev[l].rhs.alloc(len); }
        if (l < T) { W.lev[l].res.alloc(len); W.lev[l].tmp.alloc(len); }
        if (l < T && h.lev[l].sm_type == AMGX_SM_CHEBY) W.lev[l].d.alloc(len);
      }
    }
    if (down_flag)                                              // (a call without the bit may have built the work space first)
      for (int l = 0; l < top(); ++l) {
        const int64_t need = down_slots(h.lev[l], level_down(l)) * w;
        if ((int64_t)W.lev[l].part.n < need) W.lev[l].part.alloc((size_t)need);
      }
    return W;
  }

  // ------------------------------------------------------------------ launches
  // Handle::product on w = 2 or 4 interleaved vectors.  sm_pass: a product of the cycle on a level (EP_CHEB steps, the residual
  // after smoothing), which reads the single-precision image where the level has one; amgx_matvec_multi and the level-0 product
  // of amgx_pcg_multi never pass it.
  template <int EP>
  void spmm(int w, const DevMatrix& M, const double* x, double* y, const EpArgs& ep, bool sm_pass = false) {
    if (w == 2) h.product<2, EP>(M, x, y, ep, Span(), sm_pass);
    else if (w == 4) h.product<4, EP>(M, x, y, ep, Span(), sm_pass);
    else throw Err("multi-vector product: width must be 2 or 4");
  }
  // x = c * Dinv * b on w interleaved vectors of a level (scalar or block)
  void diag(int w, const DevLevel& V, const double* b, double* x, double c) {
    if (V.n == 0) return;
    if (V.bs == 1) { launch(multi_diag_kernel, Handle::grid_for(V.n * w), BLOCK, 0, h.stream, V.n * w, w == 2 ? 1 : 2, V.dinv.p, b, x, c); return; }
    auto run = [&](auto BS) { launch(multi_bdiag_kernel<BS()>, Handle::grid_for(V.n * w), BLOCK, 0, h.stream, V.n, w, V.dinv.p, b, x, c); };
    if (!dispatch<2, 3, 6>(V.bs, run)) throw Err("multi-vector cycle: unsupported block size " + std::to_string(V.bs));
  }
  void gemm(int w, int n, int ld, const double* M, const double* x, double* y) {
    if (n <= 0) return;
    const int grid = Handle::wave_grid(n);
    auto run = [&](auto W) { launch(dense_gemm_nv_kernel<W()>, grid, BLOCK, 0, h.stream, n, ld, M, x, y); };
    if (!dispatch<2, 4>(w, run)) throw Err("multi-vector dense product: width must be 2 or 4");
  }
  // columns c0 .. c0 + w of a caller's multi-vector <-> w interleaved vectors
  void pack(int64_t n, int w, const MultiView& src, int c0, double* dst) {
    if (n <= 0) return;
    launch(multi_pack_kernel, Handle::grid_for(n * w), BLOCK, 0, h.stream, n, w, src.p, src.rs, src.cs, c0, dst);
  }
  void unpack(int64_t n, int w, const double* src, const MultiView& dst, int c0) {
    if (n <= 0) return;
    launch(multi_unpack_kernel, Handle::grid_for(n * w), BLOCK, 0, h.stream, n, w, src, dst.p, dst.rs, dst.cs, c0);
  }

  // Gauss-Seidel on w interleaved vectors of a level that Handle::multi_sweep_ok or multi_block_sweep_ok admits
  template <class F>
  static void width(int w, F&& run) {
    if (!dispatch<2, 4>(w, run)) throw Err("multi-vector Gauss-Seidel: width must be 2 or 4");
  }
  // one sweep on the iterate `cur`; returns the buffer that holds the result (Handle::sweep: `oth` for the out-of-place hybrid forms)
  double* gs_sweep(int w, const DevLevel& V, int dir, double* cur, double* oth, const double* b) {
    if (V.n == 0) return cur;
    double* out = nullptr;
    width(w, [&](auto W) { out = h.sweep<W()>(V, dir, cur, oth, b); });
    return out;
  }
  // forward sweep from zero b -> x, then res = b - A x by the identity the level's images allow on w vectors (Handle::split_identity)
  void gs_down(int w, const DevLevel& V, const double* b, double* x, double* res) {
    if (V.n == 0) return;
    width(w, [&](auto W) { h.sweep_from_zero<W()>(V, x, b, res); h.residual_after_zero<W()>(V, x, b, res); });
  }

  // the residual after the sweep from zero and its restriction through the single-vector functions, column by column of a group
  // (x, b: w interleaved vectors of level l; bc: of level l + 1).  The column buffers are those of fit_cols.
  void down_cols(int w, int l, const double* b, const double* x, double* bc) {
    DevLevel& V = h.lev[l];
    const int64_t n = V.len(), nc = h.lev[l + 1].len();
    fit_cols();
    double *b1 = st.col_in.p, *x1 = st.col_out.p, *c1 = st.dn_col.p, *r = st.sm_r.p;
    for (int j = 0; j < w; ++j) {
      pack(n, 1, MultiView(b, w, 0, true), j, b1);
      pack(n, 1, MultiView(x, w, 0, true), j, x1);
      h.zero(r, n);                                            // (the multicolour identity writes swept rows only)
      if (V.paths.down == DOWN_GSB) h.residual_restrict_after_zero(l, x1, b1, r, c1);
      else { h.residual_after_zero(V, x1, b1, r); h.transfer_f2c(l, r, c1); }
      unpack(nc, 1, c1, MultiView(bc, w, 0, true), j);
    }
  }

  // b_c = P^T r through the single-vector restriction, column by column of a group (r: level l; bc: level l + 1)
  void restrict_cols(int w, int l, const double* r, double* bc) {
    const int64_t n = h.lev[l].len(), nc = h.lev[l + 1].len();
    fit_cols();
    double *r1 = st.col_in.p, *c1 = st.dn_col.p;
    for (int j = 0; j < w; ++j) {
      pack(n, 1, MultiView(r, w, 0, true), j, r1);
      h.transfer_f2c(l, r1, c1);
      unpack(nc, 1, c1, MultiView(bc, w, 0, true), j);
    }
  }
  // t = x + P x_c through the single-vector product, column by column of a group (x, t: level l; xc: level l + 1; t may be x)
  void up_cols(int w, int l, const double* xc, const double* x, double* t) {
    DevLevel& V = h.lev[l];
    const int64_t n = V.len(), nc = h.lev[l + 1].len();
    fit_cols();
    double *c1 = st.dn_col.p, *x1 = st.col_out.p, *t1 = st.sm_r.p;
    for (int j = 0; j < w; ++j) {
      pack(nc, 1, MultiView(xc, w, 0, true), j, c1);
      pack(n, 1, MultiView(x, w, 0, true), j, x1);
      h.mult_add(V.P, 1.0, c1, x1, t1);
      unpack(n, 1, t1, MultiView(t, w, 0, true), j);
    }
  }

  void coarse_multi(int w, const double* rhs, double* x) {
    const DevLevel& V = h.lev.back();
    if (h.clev != AMGX_CLEV_INV || h.coarse_n == 0) { h.zero(x, V.len() * w); return; }
    gemm(w, (int)h.coarse_n, (int)h.coarse_ld, h.coarse_inv.p, rhs, x);
  }

  // one Chebyshev smooth of a level on w interleaved vectors, from zero or from an iterate placed by cheb_place: cheb_schedule
  // with the diagonal as the step from zero and the EP_CHEB product as every other step
  void cheb(int w, const DevLevel& V, ChebEntry entry, const double* src, double* x, const double* b, double* tmp, double* d) {
    auto first = [&](const double* v, const double*, double* xout, double*, double c0) { diag(w, V, v, xout, c0); };
    auto step = [&](const double* xin, double* xout, double c1, double c2, const double* d_old, double* d_new) {
      spmm<EP_CHEB>(w, V.A, xin, xout, EpArgs{b, xin, V.dinv.p, c2, d_new, 0, d_old, c1}, true);
    };
    if (cheb_schedule(V.cheb_degree, V.cheb_c0, V.cheb_c1, V.cheb_c2, entry, b, src, x, tmp, d, first, step) != x)
      throw Err("multi-vector cycle: the Chebyshev smooth did not end in x");
  }

  // the literal V-cycle on w interleaved vectors (stage order of pre_smooth / transfer_f2c / post_smooth without folding)
  void cycle_v_multi(int w, double* x, const double* b) {
    const int L = h.n_levels();
    if (h.dense_level == 0) { gemm(w, h.dense_n, h.dense_ld, h.dense_op.p, b, x); return; }
    if (L == 1) { coarse_multi(w, b, x); return; }
    MultiWork& W = work(w);
    const int T = top();
    const EpArgs none{nullptr, nullptr, nullptr, 0.0, nullptr, 0};
    for (int l = 0; l < T; ++l) {
      const DevLevel& V = h.lev[l];
      double* xl = l == 0 ? x : W.lev[l].x.p;
      const double* bl = l == 0 ? b : W.lev[l].rhs.p;
      double* const tmp = W.lev[l].tmp.p;
      // AMGX_MULTI_FUSE_DOWN: r = b - A x stays in LDS, chunk-local P^T r from there, then the sum (Handle::down_launch_nv)
      const DownNv dn = level_down(l);
      double* const part = W.lev[l].part.p;
      double* const bc = W.lev[l + 1].rhs.p;
      if (V.sm_type == AMGX_SM_GS) {                           // sweep from zero and the residual by the level's identity
        if (dn.form) {                                         // (hybrid form with the split: r = c .* x - rest x)
          width(w, [&](auto NV) { h.sweep_from_zero<NV()>(V, xl, bl, nullptr); });
          down_nv(w, l, dn, Handle::down_ops_gsb(V, xl), part, bc);
          continue;
        }
        if (col_block(l) && res_fused(l)) {                    // (fused sweep and residual on the BSELL images, P^T per column)
          gs_down(w, V, bl, xl, W.lev[l].res.p);
          restrict_cols(w, l, W.lev[l].res.p, bc);
          continue;
        }
        if (col_down(l) || col_block(l)) {                     // (residual + restriction as the single-vector cycle runs them, per column)
          width(w, [&](auto NV) { h.sweep_from_zero<NV()>(V, xl, bl, W.lev[l].res.p); });
          down_cols(w, l, bl, xl, bc);
          continue;
        }
        gs_down(w, V, bl, xl, W.lev[l].res.p);
        spmm<EP_MULT>(w, V.PT, W.lev[l].res.p, W.lev[l + 1].rhs.p, none);
        continue;
      }
      if (V.sm_type == AMGX_SM_CHEBY) {                        // cheb_smooth from zero per column
        cheb(w, V, ChebEntry::ZERO, xl, xl, bl, tmp, W.lev[l].d.p);
        if (dn.form) { down_nv(w, l, dn, h.down_ops_cheb(xl, bl), part, bc); continue; }
      } else if (dn.form) {                                    // x = w Dinv b (z on a level whose way up is Q), r = b - A' b in one pass
        down_nv(w, l, dn, h.down_ops_jacobi(V, bl, xl, dn.fold), part, bc);
        continue;
      } else diag(w, V, bl, xl, V.omega);
      spmm<EP_RES>(w, V.A, xl, W.lev[l].res.p, EpArgs{bl, nullptr, nullptr, 0.0, nullptr, 0}, true);
      spmm<EP_MULT>(w, V.PT, W.lev[l].res.p, W.lev[l + 1].rhs.p, none);
    }
    if (h.dense_level > 0) gemm(w, h.dense_n, h.dense_ld, h.dense_op.p, W.lev[T].rhs.p, W.lev[T].x.p);
    else if (tail_cols()) {                                    // the tail program of the single-vector cycle, column by column
      const DevLevel& V = h.lev[T];
      const MultiView rhs(W.lev[T].rhs.p, w, 0, true), xt(W.lev[T].x.p, w, 0, true);
      for (int j = 0; j < w; ++j) {
        pack(V.len(), 1, rhs, j, V.rhs.p);
        launch(tail_kernel, 1, TAIL_BLOCK, 0, h.stream, h.tail_ops, h.tail_prog.p);
        unpack(V.len(), 1, V.x.p, xt, j);
      }
    } else if (col_coarse()) {                                 // the coarsest solve of the single-vector cycle, column by column
      const int64_t nT = h.lev[T].len();
      fit_cols();
      for (int j = 0; j < w; ++j) {
        pack(nT, 1, MultiView(W.lev[T].rhs.p, w, 0, true), j, st.col_in.p);
        h.coarse_solve(st.col_in.p, st.col_out.p);
        unpack(nT, 1, st.col_out.p, MultiView(W.lev[T].x.p, w, 0, true), j);
      }
    } else coarse_multi(w, W.lev[T].rhs.p, W.lev[T].x.p);
    for (int l = T - 1; l >= 0; --l) {
      const DevLevel& V = h.lev[l];
      double* xl = l == 0 ? x : W.lev[l].x.p;
      const double* bl = l == 0 ? b : W.lev[l].rhs.p;
      double* const tmp = W.lev[l].tmp.p;
      if (V.sm_type == AMGX_SM_GS) {                           // t = x + P x_c, backward sweep t -> x (in place: t = x)
        double* t = V.paths.in_place ? xl : tmp;
        if (col_block(l)) up_cols(w, l, W.lev[l + 1].x.p, xl, t);
        else spmm<EP_AXPY>(w, V.P, W.lev[l + 1].x.p, t, EpArgs{nullptr, xl, nullptr, 1.0, nullptr, 0});
        if (gs_sweep(w, V, 1, t, xl, bl) != xl) throw Err("multi-vector cycle: the Gauss-Seidel sweep did not end in x");
      } else if (V.sm_type == AMGX_SM_CHEBY) {                 // t = x + P x_c where the last of the k passes lands in x
        double* t = cheb_place(cheb_passes(V.cheb_degree, ChebEntry::ITERATE), xl, tmp);
        spmm<EP_AXPY>(w, V.P, W.lev[l + 1].x.p, t, EpArgs{nullptr, xl, nullptr, 1.0, nullptr, 0});
        cheb(w, V, ChebEntry::ITERATE, t, xl, bl, tmp, W.lev[l].d.p);
      } else if (level_down(l).fold) {                         // x = z + Q x_c (fold_prolongation): the down pass stored z
        spmm<EP_AXPY>(w, V.Q, W.lev[l + 1].x.p, xl, EpArgs{nullptr, xl, nullptr, 1.0, nullptr, 0});
      } else {
        spmm<EP_AXPY>(w, V.P, W.lev[l + 1].x.p, tmp, EpArgs{nullptr, xl, nullptr, 1.0, nullptr, 0});
        spmm<EP_JAC>(w, V.A, tmp, xl, EpArgs{bl, tmp, V.dinv.p, V.omega, nullptr, 0});
      }
    }
  }

  // one application through the single-vector path on contiguous device vectors (what amgx_apply does with device pointers)
  void apply_single(const double* b, double* x, bool graph_ok, bool capturing) {
    if (capturing) { h.do_cycle(x, b); return; }              // (fused handles only: never renumbered)
    Staged sg(h, AMGX_DEVICE_PTR);
    const int64_t n = h.lev[0].len();
    const double* db = sg.in(0, b, n, 0);
    double* dx = sg.inout(1, x, n, false, 0);
    h.run_cycle(dx, db, graph_ok);
    sg.out(1, x, n, 0);
  }

  // One walk over the column groups of a call, multi_groups(k, fused).  Per group every argument becomes ONE pointer q[i]: a
  // contiguous column (`one`) or w interleaved vectors (`group`).  Inputs are packed before the body in the order of `a`, outputs
  // unpacked from q[i] after it; a body whose result lands in another buffer sets q[i] to it.
  template <size_t N, class One, class Group>
  void walk(int k, bool fused, const MultiArg (&a)[N], One&& one, Group&& group) {
    int32_t wd[MULTI_MAX];
    const int ng = multi_groups(k, fused, wd);
    int c0 = 0;
    for (int g = 0; g < ng; c0 += wd[g], ++g) {
      const int w = wd[g];
      double* q[N];
      bool staged[N];
      MultiWork* W = nullptr;
      for (size_t i = 0; i < N; ++i) {
        const MultiArg& s = a[i];
        DevBuf<double>* buf = w == 1 ? s.col : s.grp;
        int64_t len = w == 1 ? s.col_len : s.rows * (MULTI_MAX / 2);
        staged[i] = w == 1 ? s.v.rs != 1 : true;
        if (w > 1 && !s.grp) {
          if (!W) W = &work(w);
          buf = s.role & MULTI_ARG_IN ? &W->in : &W->out;
          len = h.lev[0].len() * w;                            // (sized for level 0, the largest level)
          // an interleaved argument of exactly this width (16-byte aligned) is used in place
          staged[i] = !(k == w && s.v.rs == w && s.v.cs == 1 && (reinterpret_cast<uintptr_t>(s.v.p) & 15) == 0);
        }
        if (staged[i]) fit(*buf, len);
        q[i] = staged[i] ? buf->p : s.v.p + c0 * s.v.cs;
        if (staged[i] && (s.role & MULTI_ARG_IN)) pack(s.rows, w, s.v, c0, q[i]);
      }
      if (w == 1) one(q);
      else group(w, q);
      for (size_t i = 0; i < N; ++i)
        if (staged[i] && (a[i].role & MULTI_ARG_OUT)) unpack(a[i].rows, w, q[i], a[i].v, c0);
    }
  }

  // X = C B on device multi-vectors
  void apply_body(int k, const MultiView& B, const MultiView& X, bool graph_ok, bool capturing) {
    const int64_t n = h.lev[0].len();
    const MultiArg a[2] = {{MULTI_ARG_IN, B, n, &st.col_in, n, nullptr}, {MULTI_ARG_OUT, X, n, &st.col_out, n, nullptr}};
    walk(k, fz, a, [&](auto& q) { apply_single(q[0], q[1], graph_ok, capturing); }, [&](int w, auto& q) { cycle_v_multi(w, q[1], q[0]); });
  }

  void apply(int k, const double* B, int64_t ldb, double* X, int64_t ldx, bool interleaved, bool graph_ok) {
    const MultiView vb(B, k, ldb, interleaved), vx(X, k, ldx, interleaved);
    // only the fused path is captured as a whole; the column loop replays the single-vector graphs of run_cycle
    if (!fz || !(h.use_graph && graph_ok) || h.stream == nullptr) { apply_body(k, vb, vx, graph_ok, false); return; }
    const MultiState::Key key{B, X, k, interleaved ? 1 : 0, interleaved ? 0 : ldb, interleaved ? 0 : ldx, rule() + (down_active() ? 4 : 0) + (dia_active() ? 8 : 0) + (f32_active() ? 16 : 0) + (d32_active() ? 32 : 0)};
    if (!st.graphs.has(key)) {
      int32_t wd[MULTI_MAX];
      const int ng = multi_groups(k, true, wd);
      for (int g = 0; g < ng; ++g) {                           // allocations happen before the capture
        if (wd[g] > 1) { MultiWork& W = work(wd[g]); fit(W.in, h.lev[0].len() * wd[g]); fit(W.out, h.lev[0].len() * wd[g]); }
        else { fit(st.col_in, h.lev[0].len()); fit(st.col_out, h.lev[0].len()); }
      }
      if (col_stages()) fit_cols();
    }
    st.graphs.run(key, h.stream, [&] { apply_body(k, vb, vx, false, true); });
  }

  // Y = A_level X on device multi-vectors
  void matvec(int level, int k, const double* X, int64_t ldx, double* Y, int64_t ldy, bool interleaved) {
    const DevLevel& V = h.lev[level];
    const int64_t n = V.len(), nx = V.ext_len(), n0 = h.lev[0].len();
    // (X has ext_len rows; a handle that runs fused groups has no ghost columns, there ext_len == len)
    const MultiArg a[2] = {{MULTI_ARG_IN, MultiView(X, k, ldx, interleaved), nx, &st.col_in, std::max(nx, n0), nullptr},
                           {MULTI_ARG_OUT, MultiView(Y, k, ldy, interleaved), n, &st.col_out, std::max(n, n0), nullptr}};
    walk(k, fz, a,
         [&](auto& q) {                                        // amgx_matvec with device pointers
           Staged sg(h, AMGX_DEVICE_PTR);
           const double* dx = sg.in(0, q[0], nx, level);
           double* dy = sg.inout(1, q[1], n, false, level);
           h.mult(V.A, dx, dy);
           sg.out(1, q[1], n, level);
         },
         [&](int w, auto& q) { spmm<EP_MULT>(w, V.A, q[0], q[1], EpArgs{nullptr, nullptr, nullptr, 0.0, nullptr, 0}); });   // (no sm_pass: the fp64 image)
  }

  // one plain smoother step per column on a level (amgx_smooth per column).  Groups of 4 and 2 run the multi-vector sweeps where
  // the call carries AMGX_MULTI_FUSE_GS and the level has them (Handle::multi_sweep_ok, caller's numbering; with
  // AMGX_MULTI_FUSE_GS_BLOCK also Handle::multi_block_sweep_ok on a square-block level); everything else is a
  // column loop over level_smooth.  x_zero is the caller's promise of the flag contract; like the single-vector Gauss-Seidel
  // step, the sweeps do not act on it (they read x), so the columns of a group and the single columns see the same operation.
  void smooth(int level, int dir, int k, double* X, int64_t ldx, const double* B, int64_t ldb, bool interleaved, bool x_zero) {
    DevLevel& V = h.lev[level];
    const int64_t n = V.len(), col = std::max(n, h.lev[0].len());
    if (V.n != V.ncols) throw Err("amgx_smooth_multi: rank-partitioned levels are not supported");
    const MultiLevelFacts& f = st.facts[fb][level];
    const bool nv = gs_flag && !f.permuted && !f.empty && (f.sweep_ok || (block_flag && f.block_sweep_ok && f.block_sweep_fits));
    const MultiArg a[2] = {{MULTI_ARG_IN | MULTI_ARG_OUT, MultiView(X, k, ldx, interleaved), n, &st.col_out, col, &st.sm_x},
                           {MULTI_ARG_IN, MultiView(B, k, ldb, interleaved), n, &st.col_in, col, &st.sm_b}};
    walk(k, nv, a,
         [&](auto& q) {                                        // amgx_smooth with device pointers
           fit(st.sm_r, n);
           Staged sg(h, AMGX_DEVICE_PTR);
           double* dx = sg.inout(0, q[0], n, true, level);
           const double* db = sg.in(1, q[1], n, level);
           double* dr = sg.inout(2, st.sm_r.p, n, false, level);
           h.level_smooth(V, dir, dx, db, dr, false, false, x_zero);
           sg.out(0, q[0], n, level);
         },
         [&](int w, auto& q) {                                 // (the result is in x or in the sweep's other buffer)
           fit(st.sm_t, n * (MULTI_MAX / 2));
           q[0] = gs_sweep(w, V, dir, q[0], st.sm_t.p, q[1]);
         });
  }

  // the down stage of a level per column (amgx_down_multi): x_given = false: pre-smoothing from zero b -> x, then b_c = P^T (b - A x)
  // (Handle::pre_smooth_restrict with the level's fold); x_given = true: only the residual + restriction half on the caller's x.
  // Groups of 4 and 2 run Handle::down_launch_nv where the call carries AMGX_MULTI_FUSE_DOWN and the level takes it (level_down; a
  // Gauss-Seidel sweep from zero also needs AMGX_MULTI_FUSE_GS); everything else is a column loop over the single-vector functions.
  void down(int level, int k, const double* B, int64_t ldb, double* X, int64_t ldx, double* BC, int64_t ldbc, bool interleaved, bool x_given) {
    DevLevel& V = h.lev[level];
    const int64_t n = V.len(), nc = h.lev[level + 1].len(), col = std::max(n, h.lev[0].len());
    const bool gs = V.sm_type == AMGX_SM_GS, cheby = V.sm_type == AMGX_SM_CHEBY, jacobi = V.sm_type == AMGX_SM_JACOBI;
    if (x_given && jacobi && V.paths.jacobi_down()) throw Err("amgx_down_multi: x_given on a Jacobi level with a fused down pass (the Jacobi down pass forms x itself)");
    const DownNv dn = level_down(level);
    // AMGX_MULTI_FUSE_F32: a Gauss-Seidel level with single-precision images keeps the literal stages (level_down),
    // but with AMGX_MULTI_FUSE_GS its sweep from zero runs on the group; residual and restriction follow per column
    const MultiLevelFacts& f = st.facts[fb][level];
    // (AMGX_MULTI_FUSE_DOWN_F32, DESIGN.md 5.23: where the level has a form under the call's flags, the NV down launch comes first)
    const bool sweep32 = !x_given && gs && down_flag && gs_flag && f.f32_ok && f.sweep_ok && !f.permuted && !f.empty && !dn.form;
    const bool nv = sweep32 || (dn.form != 0 && (x_given || !gs || gs_flag));
    const MultiArg a[3] = {{MULTI_ARG_IN, MultiView(B, k, ldb, interleaved), n, &st.col_in, col, &st.sm_b},
                           {x_given ? MULTI_ARG_IN : MULTI_ARG_OUT, MultiView(X, k, ldx, interleaved), n, &st.col_out, col, &st.sm_x},
                           {MULTI_ARG_OUT, MultiView(BC, k, ldbc, interleaved), nc, &st.dn_col, nc, &st.dn_c}};
    walk(k, nv, a,
         [&](auto& q) {                                        // the single-vector functions with device pointers
           const double* b1 = q[0];
           double *x1 = q[1], *c1 = q[2];
           fit(st.sm_r, n);
           double* const r = st.sm_r.p;
           if (!x_given) h.pre_smooth_restrict(level, x1, b1, r, c1, h.folded(V));
           else if (cheby && V.paths.down == DOWN_CHEB) h.down_launch(level, V.plan_rf, h.down_ops_cheb(x1, b1), c1);
           else if (gs && V.paths.down == DOWN_GSB) h.residual_restrict_after_zero(level, x1, b1, r, c1);
           else { h.residual_sm(V, x1, b1, r); h.transfer_f2c(level, r, c1); }
         },
         [&](int w, auto& q) {
           constexpr int WMAX = MULTI_MAX / 2;                 // the widest group
           fit(st.sm_t, n * WMAX); fit(st.dn_d, n * WMAX); fit(st.dn_part, down_slots(V, dn) * WMAX);
           double *bw = q[0], *xw = q[1];
           if (sweep32) {
             width(w, [&](auto NV) { h.sweep_from_zero<NV()>(V, xw, bw, st.sm_t.p); });
             down_cols(w, level, bw, xw, q[2]);                // the single-vector residual and restriction of every column
             return;
           }
           if (!x_given && cheby) cheb(w, V, ChebEntry::ZERO, xw, xw, bw, st.sm_t.p, st.dn_d.p);
           else if (!x_given && gs) width(w, [&](auto NV) { h.sweep_from_zero<NV()>(V, xw, bw, nullptr); });
           if (jacobi) down_nv(w, level, dn, h.down_ops_jacobi(V, bw, xw, h.folded(V)), st.dn_part.p, q[2]);
           else if (cheby) down_nv(w, level, dn, h.down_ops_cheb(xw, bw), st.dn_part.p, q[2]);
           else down_nv(w, level, dn, Handle::down_ops_gsb(V, xw), st.dn_part.p, q[2]);
         });
  }

  // k independent preconditioned CG recurrences (Krylov::pcg per column) that share the operator product and the preconditioner
  // application.  B, X: device multi-vectors.
  void pcg(int k, const MultiView& B, const MultiView& X, double tol, int maxit, bool use_pre, bool graph_ok, double* errs, int32_t* iters) {
    if (h.lev[0].n != h.lev[0].ncols) throw Err("Krylov solvers need a square level-0 matrix (single rank)");
    const int64_t n = h.lev[0].len(), len = n * k;
    for (auto& v : st.kr) fit(v, len);
    if (st.kr_sc.n < (size_t)3 * MULTI_MAX) { st.kr_sc.alloc(3 * MULTI_MAX); st.kr_partial.alloc((size_t)KR_BLOCKS * MULTI_MAX); st.kr_active.alloc(MULTI_MAX); }
    double *b = st.kr[0].p, *x = st.kr[1].p, *d = st.kr[2].p, *w = st.kr[3].p, *s = st.kr[4].p;
    double* sc = st.kr_sc.p;                                  // rows of MULTI_MAX scalars: 0 / 1 = <w, d> of the last two iterations, 2 = <s, A s>
    const int nb = (int)std::max<int64_t>(1, std::min<int64_t>(KR_BLOCKS, (n + BLOCK - 1) / BLOCK));
    const int grid = Handle::grid_for(len);
    hipStream_t sm = h.stream;
    auto dot = [&](const double* a, const double* c, int slot) {
      launch(kr_dot_multi_partial_kernel, nb, BLOCK, 0, sm, n, k, a, c, st.kr_partial.p);
      launch(kr_dot_final_kernel, k, BLOCK, 0, sm, nb, st.kr_partial.p, sc + slot * MULTI_MAX);
    };
    auto read = [&](int slot, double* out) {
      HIPCHK(hipMemcpyAsync(out, sc + slot * MULTI_MAX, k * sizeof(double), hipMemcpyDeviceToHost, sm));
      HIPCHK(hipStreamSynchronize(sm));
    };
    auto precond = [&](const double* r, double* z) {
      if (use_pre) apply(k, r, 0, z, 0, true, graph_ok);
      else h.copy(z, r, len);
    };
    int32_t active[MULTI_MAX];
    auto push_active = [&]() {
      HIPCHK(hipMemcpyAsync(st.kr_active.p, active, k * sizeof(int32_t), hipMemcpyHostToDevice, sm));
      HIPCHK(hipStreamSynchronize(sm));                       // (the host array changes again before the next copy)
    };
    pack(n, k, B, 0, b);
    pack(n, k, X, 0, x);
    matvec(0, k, x, 0, w, 0, true);                           // d = b - A x
    launch(multi_sub_kernel, grid, BLOCK, 0, sm, len, b, w, d);
    precond(d, w);
    h.copy(s, w, len);
    int cur = 1;
    dot(w, d, cur);
    double err0[MULTI_MAX], v[MULTI_MAX];
    read(cur, v);
    int n_active = 0;
    for (int j = 0; j < k; ++j) {
      err0[j] = std::sqrt(std::fabs(v[j]));
      if (errs) errs[(size_t)j * (maxit + 1)] = err0[j];
      iters[j] = 0;
      active[j] = err0[j] != 0.0 && maxit > 0;                // (NaN: the column iterates to maxit, like amgx_pcg)
      n_active += active[j];
    }
    push_active();
    for (int it = 1; it <= maxit && n_active > 0; ++it) {
      matvec(0, k, s, 0, w, 0, true);                         // w = A s
      const int old = cur;
      cur = 1 - cur;
      dot(s, w, 2);
      launch(kr_cg_update_multi_kernel, grid, BLOCK, 0, sm, len, k, sc + old * MULTI_MAX, sc + 2 * MULTI_MAX, st.kr_active.p, s, w, x, d);
      precond(d, w);
      dot(w, d, cur);
      launch(kr_xpby_multi_kernel, grid, BLOCK, 0, sm, len, k, sc + cur * MULTI_MAX, sc + old * MULTI_MAX, st.kr_active.p, w, s);
      read(cur, v);                                           // k scalars per iteration, one copy
      bool changed = false;
      for (int j = 0; j < k; ++j) {
        if (!active[j]) continue;
        const double err = std::sqrt(std::fabs(v[j]));
        if (errs) errs[(size_t)j * (maxit + 1) + it] = err;
        iters[j] = it;
        if (err <= tol * err0[j]) { active[j] = 0; --n_active; changed = true; }    // frozen: its x is not touched again
      }
      if (changed && n_active > 0) push_active();
    }
    unpack(n, k, x, X, 0);
  }
};

// host-pointer arguments of the multi-vector calls: one staged copy per multi-vector, laid out as the caller's (column-major
// copies are compacted to ld = rows)
struct MultiStaged {
  Handle& h;
  bool host;
  MultiStaged(Handle& hh, int flags) : h(hh), host(!(flags & AMGX_DEVICE_PTR)) {}
  const double* in(DevBuf<double>& buf, const double* p, int64_t rows, int k, bool interleaved, int64_t ld, bool load = true) {
    if (!host) return p;
    // (sized once for the widest call: the graphs of apply() are keyed on the address, which must not move when k grows)
    Multi::fit(buf, std::max<int64_t>(rows * k, h.lev[0].ext_len() * MULTI_MAX));
    if (load) {
      if (interleaved || ld == rows) HIPCHK(hipMemcpyAsync(buf.p, p, (size_t)rows * k * sizeof(double), hipMemcpyHostToDevice, h.stream));
      else for (int j = 0; j < k; ++j) HIPCHK(hipMemcpyAsync(buf.p + j * rows, p + j * ld, (size_t)rows * sizeof(double), hipMemcpyHostToDevice, h.stream));
    }
    return buf.p;
  }
  void out(const DevBuf<double>& buf, double* p, int64_t rows, int k, bool interleaved, int64_t ld) {
    if (!host) return;
    if (interleaved || ld == rows) HIPCHK(hipMemcpyAsync(p, buf.p, (size_t)rows * k * sizeof(double), hipMemcpyDeviceToHost, h.stream));
    else for (int j = 0; j < k; ++j) HIPCHK(hipMemcpyAsync(p + j * ld, buf.p + j * rows, (size_t)rows * sizeof(double), hipMemcpyDeviceToHost, h.stream));
    HIPCHK(hipStreamSynchronize(h.stream));
  }
};

// One multi-vector argument of a C entry point: the caller's pointer and leading dimension, its rows, its staged copy in a
// host-pointer call, and whether that copy is loaded before / stored after the call.
struct MultiCallArg { const double* p; int64_t ld, rows; DevBuf<double> MultiState::* stage; bool load, store; };

// What every amgx_*_multi entry point does around its one call: the checks of its multi-vectors under its name (`also`: the
// entry's complaint about its other arguments, raised after them), Multi, the staged copies of host arrays with their compact
// leading dimension, and the way back of the outputs.  body(M, d, ld, interleaved): device pointers and leading dimensions.
template <size_t N, class F>
void multi_call(const char* fn, Handle& h, int k, int flags, const MultiCallArg (&a)[N], const char* also, F&& body) {
  const std::string f(fn);
  const bool il = flags & AMGX_MULTI_INTERLEAVED;
  if (k < 1 || k > MULTI_MAX) throw Err(f + ": k must be 1 .. " + std::to_string(MULTI_MAX) + " (got " + std::to_string(k) + ")");
  for (size_t m = 2; m <= N; ++m) {       // the first two arguments, then each further one
    for (size_t i = 0; i < m; ++i) if (!a[i].p) throw Err(f + ": null multi-vector");
    for (size_t i = 0; i < m; ++i) for (size_t j = 0; j < i; ++j) if (a[i].p == a[j].p) throw Err(f + ": the multi-vectors must not alias");
    for (size_t i = 0; i < m; ++i) if (!il && k > 1 && a[i].ld < a[i].rows) throw Err(f + ": leading dimension below the level size");
  }
  if (also) throw Err(f + ": " + also);
  Multi M(h, flags);
  MultiStaged sg(h, flags);
  double* d[N];
  int64_t ld[N];
  for (size_t i = 0; i < N; ++i) {
    d[i] = const_cast<double*>(sg.in(M.st.*a[i].stage, a[i].p, a[i].rows, k, il, a[i].ld, a[i].load));
    ld[i] = (sg.host && !il) ? a[i].rows : a[i].ld;            // (staged copies are compact)
  }
  body(M, d, ld, il);
  for (size_t i = 0; i < N; ++i) if (a[i].store) sg.out(M.st.*a[i].stage, const_cast<double*>(a[i].p), a[i].rows, k, il, a[i].ld);
}

// the note functions: the text lives until the thread's next call of the same function
template <class F>
const char* multi_note_call(amgx_handle hh, F&& text) {
  thread_local std::string note;
  note.clear();
  if (guard(hh, [&](Handle& h) { note = text(h); })) note = amgx_last_error(hh);
  return note.c_str();
}

}  // namespace amgx

extern "C" {

int amgx_apply_multi(amgx_handle hh, int k, const double* B, int64_t ldb, double* X, int64_t ldx, int b_status, int flags) {
  if (k == 1 && hh && hh->h) return amgx_apply(hh, B, X, b_status, flags & ~(AMGX_MULTI_INTERLEAVED | amgx::Multi::CALL_FLAGS));   // the single-vector path itself
  (void)b_status;   // single GPU: DISTRIBUTED == CUMULATED, as in amgx_apply
  return guard(hh, [&](amgx::Handle& h) {
    const int64_t n = h.lev[0].len();
    const amgx::MultiCallArg a[2] = {{B, ldb, n, &amgx::MultiState::stage_b, true, false}, {X, ldx, n, &amgx::MultiState::stage_x, false, true}};
    amgx::multi_call("amgx_apply_multi", h, k, flags, a, nullptr,
                     [&](amgx::Multi& M, auto& d, auto& ld, bool il) { M.apply(k, d[0], ld[0], d[1], ld[1], il, !(flags & AMGX_NO_GRAPH)); });
  });
}

int amgx_matvec_multi(amgx_handle hh, int level, int k, const double* X, int64_t ldx, double* Y, int64_t ldy, int flags) {
  return guard(hh, [&](amgx::Handle& h) {
    if (level < 0 || level >= h.n_levels()) throw amgx::Err("amgx_matvec_multi: level out of range");
    const int64_t n = h.lev[level].len(), nx = h.lev[level].ext_len();
    const amgx::MultiCallArg a[2] = {{X, ldx, nx, &amgx::MultiState::stage_b, true, false}, {Y, ldy, n, &amgx::MultiState::stage_x, false, true}};
    amgx::multi_call("amgx_matvec_multi", h, k, flags, a, nullptr,
                     [&](amgx::Multi& M, auto& d, auto& ld, bool il) { M.matvec(level, k, d[0], ld[0], d[1], ld[1], il); });
  });
}

int amgx_smooth_multi(amgx_handle hh, int level, int dir, int k, double* X, int64_t ldx, const double* B, int64_t ldb, int x_zero, int flags) {
  return guard(hh, [&](amgx::Handle& h) {
    if (level < 0 || level >= h.n_levels()) throw amgx::Err("amgx_smooth_multi: level out of range");
    if (!h.lev[level].dinv.p) throw amgx::Err("amgx_smooth_multi: level has no smoother");
    const int64_t n = h.lev[level].len();
    const amgx::MultiCallArg a[2] = {{B, ldb, n, &amgx::MultiState::stage_b, true, false}, {X, ldx, n, &amgx::MultiState::stage_x, true, true}};
    amgx::multi_call("amgx_smooth_multi", h, k, flags, a, nullptr,
                     [&](amgx::Multi& M, auto& d, auto& ld, bool il) { M.smooth(level, dir, k, d[1], ld[1], d[0], ld[0], il, x_zero != 0); });
  });
}

int amgx_down_multi(amgx_handle hh, int level, int k, const double* B, int64_t ldb, double* X, int64_t ldx, double* BC, int64_t ldbc, int x_given,
                    int flags) {
  return guard(hh, [&](amgx::Handle& h) {
    if (level < 0 || level + 1 >= h.n_levels()) throw amgx::Err("amgx_down_multi: level out of range (the level must be smoothed)");
    const amgx::DevLevel& V = h.lev[level];
    if (V.bs != 1 || h.lev[level + 1].bs != 1) throw amgx::Err("amgx_down_multi: block level");
    if (!V.dinv.p) throw amgx::Err("amgx_down_multi: level has no smoother");
    if (V.n != V.ncols) throw amgx::Err("amgx_down_multi: rank-partitioned levels are not supported");
    if (h.permuted(level) || h.permuted(level + 1)) throw amgx::Err("amgx_down_multi: renumbered level");
    const int64_t n = V.len(), nc = h.lev[level + 1].len();
    const bool given = x_given != 0;
    const amgx::MultiCallArg a[3] = {{B, ldb, n, &amgx::MultiState::stage_b, true, false}, {X, ldx, n, &amgx::MultiState::stage_x, given, !given},
                                     {BC, ldbc, nc, &amgx::MultiState::stage_c, false, true}};
    amgx::multi_call("amgx_down_multi", h, k, flags, a, nullptr,
                     [&](amgx::Multi& M, auto& d, auto& ld, bool il) { M.down(level, k, d[0], ld[0], d[1], ld[1], d[2], ld[2], il, given); });
  });
}

int amgx_multi_level_plan(amgx_handle hh, int level, int flags, int32_t* out, int n_out) {
  return guard(hh, [&](amgx::Handle& h) {
    if (level < 0 || level >= h.n_levels()) throw amgx::Err("amgx_multi_level_plan: level out of range");
    if (!out || n_out < 1) throw amgx::Err("amgx_multi_level_plan: bad arguments");
    amgx::Multi M(h, flags & amgx::Multi::CALL_FLAGS);
    const amgx::Multi::DownNv d = M.level_down(level);
    const int32_t v[5] = {d.form, d.form ? d.mode : 0, d.fold ? 1 : 0, d.f32 ? 1 : 0,
                          d.form == 5  ? (int32_t)amgx::down_nv_lw_lds_bytes(*d.plan, 4)
                          : d.form >= 3 ? (int32_t)amgx::down_nv_dia_lds_bytes(*d.plan, 4) : d.form ? (int32_t)amgx::down_nv_lds_bytes(*d.plan, 4) : 0};
    for (int i = 0; i < std::min(n_out, 5); ++i) out[i] = v[i];
    // out[5 .. 7]: the shape of the level's fused down plan, whether or not a fused group takes it: lanes per row, entries of P per
    // thread, the longest column list of a local-window chunk (all 0 without a plan)
    const int32_t shape[3] = {d.plan ? d.plan->lanes : 0, d.plan ? d.plan->ept : 0, d.plan ? d.plan->lw_max_list : 0};
    for (int i = 5; i < std::min(n_out, 8); ++i) out[i] = shape[i - 5];
  });
}

const char* amgx_multi_level_note(amgx_handle hh, int level, int flags) {
  return amgx::multi_note_call(hh, [&](amgx::Handle& h) -> std::string {
    if (level < 0 || level >= h.n_levels()) throw amgx::Err("amgx_multi_level_note: level out of range");
    return amgx::Multi(h, flags & amgx::Multi::CALL_FLAGS).level_down(level).why;
  });
}

int amgx_pcg_multi(amgx_handle hh, int k, const double* B, int64_t ldb, double* X, int64_t ldx, double tol, int maxit, int use_precond, int flags,
                   double* errs, int32_t* iters) {
  return guard(hh, [&](amgx::Handle& h) {
    const int64_t n = h.lev[0].len();
    const amgx::MultiCallArg a[2] = {{B, ldb, n, &amgx::MultiState::stage_b, true, false}, {X, ldx, n, &amgx::MultiState::stage_x, true, true}};
    amgx::multi_call("amgx_pcg_multi", h, k, flags, a, (maxit < 0 || !iters) ? "bad arguments (maxit < 0 or iters == NULL)" : nullptr,
                     [&](amgx::Multi& M, auto& d, auto& ld, bool il) {
                       M.pcg(k, amgx::MultiView(d[0], k, ld[0], il), amgx::MultiView(d[1], k, ld[1], il), tol, maxit, use_precond != 0, !(flags & AMGX_NO_GRAPH), errs, iters);
                     });
  });
}

int amgx_multi_info(amgx_handle hh, int k, int32_t* fused, int32_t* n_groups, int32_t* group_width, int64_t* work_bytes) {
  return amgx_multi_plan(hh, k, 0, fused, n_groups, group_width, work_bytes);
}

int amgx_multi_plan(amgx_handle hh, int k, int flags, int32_t* fused, int32_t* n_groups, int32_t* group_width, int64_t* work_bytes) {
  return guard(hh, [&](amgx::Handle& h) {
    const std::string fn = (flags & amgx::Multi::CALL_FLAGS) ? "amgx_multi_plan" : "amgx_multi_info";
    if (k < 1 || k > amgx::MULTI_MAX) throw amgx::Err(fn + ": k must be 1 .. " + std::to_string(amgx::MULTI_MAX) + " (got " + std::to_string(k) + ")");
    amgx::Multi M(h, flags & amgx::Multi::CALL_FLAGS);
    int32_t wd[amgx::MULTI_MAX];
    const int ng = amgx::multi_groups(k, M.fz, wd);
    if (fused) *fused = M.fz ? 1 : 0;
    if (n_groups) *n_groups = ng;
    if (group_width) for (int g = 0; g < amgx::MULTI_MAX; ++g) group_width[g] = g < ng ? wd[g] : 0;
    if (work_bytes) *work_bytes = M.work_bytes(k);
  });
}

const char* amgx_multi_note(amgx_handle hh, int flags) {
  return amgx::multi_note_call(hh, [&](amgx::Handle& h) -> std::string {
    amgx::Multi M(h, flags & amgx::Multi::NOTE_FLAGS);
    return M.fz ? std::string() : M.note();
  });
}

}  // extern "C"

