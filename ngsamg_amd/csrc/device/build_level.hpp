// Construction of a Handle (amgx_create): create() is the orchestration, every image of a level is built by one named step over
// the LevelBuild context.  The steps start the concurrent host tasks of a level (SetupTasks) in the order and grouping of the
// "task" lines of AMGX_SETUP_LOG; which path a level takes is decided here, from the switches in knobs.hpp.
//
// Included from amgx.hip (after the builders it calls); not a stand-alone header.
#pragma once

namespace amgx {

// What the steps of one level share.  Declared BEFORE the task pool: the workers capture it by reference, and an exception between
// tasks.run() and tasks.wait() must join the workers -- ~SetupTasks -- before the buffers they read are freed.
struct LevelBuild {
  const Knobs& K;
  SetupClock& clk;
  const amgx_level_desc& s;             // this level ...
  const amgx_level_desc* c;             // ... and the next coarser one (null on the last level)
  DevLevel& L;
  int l;
  int cycle;
  int dense_first;                      // see create()
  int n_levels;
  // big scalar levels: the CSR arrays go to the device once and kernels write the images of A, A' and Q there (devbuild.hpp)
  DevCsrSrc csrA;
  DbDiagInfo diagA;
  bool dev_images = false, verify_images = false;
  // big square-block levels: the block-CSR arrays go to the device once, the BSELL images (A; the block-hybrid Gauss-Seidel
  // images) are gathered there
  DevBcsrSrc csrB;
  bool dev_bsell = false, verify_bsell = false;
  bool last() const { return c == nullptr; }
  // levels whose smoother runs: all but the coarsest, and the only level of a single-level handle (a stand-alone smoother)
  bool smoothed() const { return !last() || n_levels == 1; }
};

// shape and smoother-parameter validation; the scalar fields of the level
static void check_level(LevelBuild& B) {
  const amgx_level_desc& s = B.s;
  DevLevel& L = B.L;
  // n_cols > n_rows: the trailing columns are ghost entries of a rank-partitioned level (filled by the caller's
  // halo exchange before every operation that gathers from them)
  if (s.A.n_cols < s.A.n_rows || s.A.br != s.A.bc) throw Err("level matrix must have n_cols >= n_rows and square blocks");
  L.n = s.A.n_rows; L.ncols = s.A.n_cols; L.bs = s.A.br;
  L.sm_type = s.sm_type; L.omega = s.omega; L.sm_steps = s.sm_steps; L.sm_symm = s.sm_symm;
  if (s.sm_type != AMGX_SM_JACOBI && s.sm_type != AMGX_SM_GS && s.sm_type != AMGX_SM_BGS && s.sm_type != AMGX_SM_CHEBY) throw Err("unknown smoother type");
  if (s.sm_type == AMGX_SM_CHEBY) {
    const int deg = s.cheb_degree == 0 ? 2 : s.cheb_degree;
    if (deg < 1 || deg > 8) throw Err("amgx_create: cheb_degree must be 1 .. 8 (0: default 2), got " + std::to_string(s.cheb_degree));
    if (!(s.cheb_lambda_max >= 0.0)) throw Err("amgx_create: cheb_lambda_max must be >= 0 (0: estimated on the device)");
    if (s.cheb_ratio != 0.0 && !(s.cheb_ratio > 1.0)) throw Err("amgx_create: cheb_ratio must be > 1 (0: default 10)");
    // (ghost columns: only on the handle a rank-partitioned driver runs stage by stage -- dense_first < 0, amgx_dist_create)
    if (s.A.n_cols != s.A.n_rows && B.dense_first >= 0) throw Err("amgx_create: a Chebyshev level with ghost columns belongs to a rank-partitioned hierarchy (amgx_dist_create)");
    L.cheb_degree = deg;
    L.cheb_ratio = s.cheb_ratio == 0.0 ? 10.0 : s.cheb_ratio;
    if (s.cheb_lambda_max > 0.0) L.cheb_set_interval(s.cheb_lambda_max);
  }
  // single-precision matrix storage (the coarsest level of a cycle, which has no smoother passes, ignores the field)
  if (B.smoothed()) {
    if (s.mat_prec != AMGX_PREC_F64 && s.mat_prec != AMGX_PREC_F32 && s.mat_prec != AMGX_PREC_F32_SCALAR_GS)
      throw Err("amgx_create: level " + std::to_string(B.l) + ": mat_prec must be AMGX_PREC_F64 (0), AMGX_PREC_F32 (1) or AMGX_PREC_F32_SCALAR_GS (2), got " +
                std::to_string(s.mat_prec));
    // single-precision images of a scalar Gauss-Seidel level: a value of its own, AMGX_PREC_F32 keeps every error below
    if (s.mat_prec == AMGX_PREC_F32_SCALAR_GS) {
      const std::string at = "amgx_create: level " + std::to_string(B.l) + ": mat_prec = AMGX_PREC_F32_SCALAR_GS ";
      if (s.sm_type != AMGX_SM_GS) throw Err(at + "is available on Gauss-Seidel levels (sm_type = AMGX_SM_GS) only");
      if (s.A.br != 1) throw Err(at + "is available on scalar levels (block size 1) only; a square-block Gauss-Seidel level takes AMGX_PREC_F32");
      if (s.A.n_cols != s.A.n_rows || B.dense_first < 0) throw Err(at + "is not available on rank-partitioned levels");
    }
    // (AMGX_PREC_F32 on a scalar Gauss-Seidel level stays the error it was: its images are asked for with AMGX_PREC_F32_SCALAR_GS)
    if (s.mat_prec == AMGX_PREC_F32 && s.sm_type != AMGX_SM_CHEBY && !(s.sm_type == AMGX_SM_GS && s.A.br > 1))
      throw Err("amgx_create: level " + std::to_string(B.l) + ": mat_prec = AMGX_PREC_F32 is available on Chebyshev levels (sm_type = AMGX_SM_CHEBY) "
                "and on square-block Gauss-Seidel levels (sm_type = AMGX_SM_GS, block size > 1) only");
    if (s.mat_prec == AMGX_PREC_F32 && s.A.n_cols != s.A.n_rows)
      throw Err("amgx_create: level " + std::to_string(B.l) + ": mat_prec = AMGX_PREC_F32 is not available on rank-partitioned levels");
    // single-precision images of a scalar Jacobi level: a field of its own, mat_prec keeps every error above
    if (s.jacobi_prec != AMGX_JACOBI_PREC_F64) {
      const std::string at = "amgx_create: level " + std::to_string(B.l) + ": jacobi_prec ";
      if (s.jacobi_prec != AMGX_JACOBI_PREC_F32 && s.jacobi_prec != AMGX_JACOBI_PREC_F32_WIDE)
        throw Err(at + "must be AMGX_JACOBI_PREC_F64 (0), AMGX_JACOBI_PREC_F32 (1) or AMGX_JACOBI_PREC_F32_WIDE (2), got " + std::to_string(s.jacobi_prec));
      if (s.sm_type != AMGX_SM_JACOBI) throw Err(at + "is available on Jacobi levels (sm_type = AMGX_SM_JACOBI) only");
      if (s.A.br != 1) throw Err(at + "is available on scalar levels (block size 1) only, not on a block Jacobi level");
      if (s.A.n_cols != s.A.n_rows || B.dense_first < 0) throw Err(at + "is not available on rank-partitioned levels");
    }
  }
  check_matrix(s.A, "A");            // (before anything reads rowptr[n_rows]: a NULL / garbage descriptor is an error, not a crash)
}

// task "A": the image of the level matrix -- device BSELL builder, device SELL builder, host builder, in this order
static void level_matrix_task(LevelBuild& B) {
  const amgx_level_desc& s = B.s;
  DevLevel& L = B.L;
  if (B.dev_bsell) {
    if (dev_build_bsell(B.csrB, nullptr, 0, BB_ALL, DbBgsbMaps(), 0, 1.30, L.A)) {
      L.A.n_rows = s.A.n_rows; L.A.n_cols = s.A.n_cols; L.A.br = s.A.br; L.A.bc = s.A.bc;
      L.A.nnz = s.A.rowptr[s.A.n_rows];
      L.A.lanes = pick_lanes(L.A.n_rows ? (double)L.A.nnz / (double)L.A.n_rows : 0.0);
      if (B.verify_bsell) verify_level_bsell(B.K, s.A, L.A);
      return;
    }
    L.A = DevMatrix();
  }
  if (B.dev_images && dev_upload_matrix(B.K, B.csrA, L.A, true, 1.35, 0, &B.diagA)) {
    if (B.verify_images) verify_level_image(B.K, s.A, L.A);
    return;
  }
  if (B.verify_images) verify_level_declined(B.K, s.A);
  // block GS walks the CSR arrays of A, so keep A in CSR there
  upload_matrix(B.K, s.A, L.A, "A", true, true, s.sm_type == AMGX_SM_GS && s.A.br > 1 && s.gs_block_rows == 0);
}

// the CSR arrays of a big level to the device (calling thread), then task "A"
static void upload_level_matrix(LevelBuild& B, SetupTasks& tasks) {
  const amgx_level_desc& s = B.s;
  DevLevel& L = B.L;
  B.dev_images = dev_images_wanted(B.K, s.A);
  B.verify_images = B.dev_images && B.K.verify_images;
  if (B.dev_images) {
    check_matrix(s.A, "A");
    B.csrA.upload(s.A);
    if (s.dinv) L.dinv.upload(s.dinv, (size_t)(B.last() ? L.n : L.ncols) * L.bs * L.bs);
    B.diagA = dev_diag_check(B.csrA, (s.dinv && s.A.n_rows <= s.A.n_cols) ? L.dinv.p : nullptr);
    B.clk.lap("CSR of A to the device", B.l);
  }
  const bool keep_csr_A = s.sm_type == AMGX_SM_GS && s.A.br > 1 && s.gs_block_rows == 0;
  B.dev_bsell = dev_bsell_wanted(B.K, s.A) && s.A.n_rows == s.A.n_cols && !keep_csr_A;
  B.verify_bsell = B.dev_bsell && B.K.verify_images;
  if (B.dev_bsell) {
    check_matrix(s.A, "A");
    B.csrB.upload(s.A);
    B.clk.lap("block CSR of A to the device", B.l);
  }
  tasks.run([&B] { level_matrix_task(B); }, "A");
}

// task "P, PT": the transfer matrices and, where asked for, the column-blocked restriction
static void upload_transfers(LevelBuild& B, SetupTasks& tasks) {
  const amgx_level_desc &s = B.s, &c = *B.c;
  if (s.P.n_rows != s.A.n_rows || s.P.n_cols > c.A.n_cols || s.P.n_cols < c.A.n_rows || s.P.br != s.A.br || s.P.bc != c.A.br)
    throw Err("P does not match the level matrices");
  if (s.PT.n_rows != s.P.n_cols || s.PT.n_cols != s.P.n_rows || s.PT.br != s.P.bc || s.PT.bc != s.P.br)
    throw Err("PT does not match P");
  if (!s.dinv) throw Err("dinv missing");
  tasks.run([&B] {
    const amgx_level_desc& s = B.s;
    DevLevel& L = B.L;
    upload_matrix(B.K, s.P, L.P, "P", true, false, false, 1.35, s.P.br == 1 && s.P.bc == 1 ? -SELL_WIN : 0, nullptr, 1);
    upload_matrix(B.K, s.PT, L.PT, "PT", true, false, false, 1.35, 0, nullptr, 2);
    // big scalar levels restrict through the column-blocked form (the P^T gather is TA/L2-bound there)
    // Measured non-win (profiles/r01/restrict_blocked.txt): 121 + 22 us vs 134 us for the P^T gather at cfg 2,
    // so the blocked form is OFF unless AMGX_RESTRICT_MIN_ROWS asks for it (kept for the fused-residual plan).
    if (s.P.br == 1 && s.P.bc == 1 && s.P.n_rows >= B.K.restrict_min_rows && s.P.rowptr[s.P.n_rows] < I32_MAX)
      build_restrict(B.K, s.P, L.R);
  }, "P, PT");
}

// task "smoother data": dinv and the Gauss-Seidel forms
static void build_smoother_data(LevelBuild& B, SetupTasks& tasks) {
  tasks.run([&B] {
    const amgx_level_desc& s = B.s;
    DevLevel& L = B.L;
    if (!B.dev_images) L.dinv.upload(s.dinv, (size_t)L.ncols * L.bs * L.bs);
    if (s.sm_type == AMGX_SM_GS && s.gs_block_rows > 0 && s.A.br > 1) {
      build_bgsb(B.K, s, L, B.dev_bsell ? &B.csrB : nullptr);
      if (B.verify_bsell) verify_bgsb(B.K, s, L);
    }
    else if (s.sm_type == AMGX_SM_GS && s.gs_block_rows > 0) {
      build_gsb(B.K, s, L, &s.P, B.dev_images ? &B.csrA : nullptr);
      if (B.verify_images) verify_gsb(B.K, s, L);
    }
    else if (s.sm_type == AMGX_SM_GS) build_gs(B.K, s, L);
    if (s.sm_type == AMGX_SM_BGS) build_bgs(s, L);
  }, "smoother data");
}

// the coarsest level has no transfers: its smoother data on the calling thread
static void build_coarsest_smoother_data(LevelBuild& B) {
  const amgx_level_desc& s = B.s;
  DevLevel& L = B.L;
  L.dinv.upload(s.dinv, (size_t)L.n * L.bs * L.bs);
  if (s.sm_type == AMGX_SM_GS && s.color && s.gs_block_rows > 0 && s.A.br > 1) build_bgsb(B.K, s, L);
  else if (s.sm_type == AMGX_SM_GS && s.color && s.gs_block_rows > 0) build_gsb(B.K, s, L, nullptr);
  else if (s.sm_type == AMGX_SM_GS && s.color) build_gs(B.K, s, L);
  if (s.sm_type == AMGX_SM_BGS && s.bgs_n_blocks > 0) build_bgs(s, L);
}

// ---- scalar Jacobi levels: the image for the fused down pass (pre-smoothing + restriction) ----------------------------------

// dinv_i * A_ii == 1 (to 1e-13) on every row with dinv_i != 0
static bool host_diag_plain(const amgx_level_desc& s) {
  std::vector<char> notplain(setup_threads(), 0);
  par_for(s.A.n_rows, [&](int64_t i0, int64_t i1, int t) {
    for (int64_t i = i0; i < i1; ++i) {
      if (s.dinv[i] == 0.0) continue;
      double aii = 0.0;
      for (int64_t k = s.A.rowptr[i]; k < s.A.rowptr[i + 1]; ++k) if (s.A.col[k] == i) { aii = s.A.val[k]; break; }
      if (!(std::fabs(s.dinv[i] * aii - 1.0) < 1e-13)) { notplain[t] = 1; break; }
    }
  });
  for (char cc : notplain) if (cc) return false;
  return true;
}

// A' = A diag(omega Dinv) in CSR order (uninitialised allocation: every entry is written)
// (rank-partitioned levels: dinv must cover the ghost columns too, i.e. n_cols entries)
static std::unique_ptr<double[]> scaled_values(const amgx_level_desc& s) {
  const int64_t nnz = s.A.rowptr[s.A.n_rows];
  std::unique_ptr<double[]> sv(new double[(size_t)std::max<int64_t>(1, nnz)]);
  par_for(nnz, [&](int64_t k0, int64_t k1, int) { for (int64_t k = k0; k < k1; ++k) sv[k] = s.A.val[k] * (s.omega * s.dinv[s.A.col[k]]); }, 1 << 16);
  return sv;
}

// long-row levels (>= 1) of a reference-shaped hierarchy: the "local window" image for the fused down kernel
static bool lw_image(LevelBuild& B) {
  const amgx_level_desc& s = B.s;
  DevLevel& L = B.L;
  const int64_t nnzA = s.A.rowptr[s.A.n_rows];
  const double avgA = s.A.n_rows ? (double)nnzA / (double)s.A.n_rows : 0.0;
  // (rank-partitioned levels too: the window of an interior chunk holds owned columns only, ghost columns are just columns)
  if (B.l == 0 || avgA < 24.0 || !B.K.lw_wanted(s.A.n_rows) || !B.K.fused_restrict_ok(s.P, 1)) return false;
  // two lanes per row (256-row chunks); levels whose 256-row chunks touch too many columns: four lanes (128-row chunks)
  int G = 0;
  std::unique_ptr<double[]> sv;
  auto host_lw = [&](int g, DevMatrix& M, DevBuf<int32_t>& cp, DevBuf<int32_t>& cc) {
    if (!sv) sv = scaled_values(s);
    return build_sell_lw(B.K, s.A, sv.get(), g, M, cp, cc);
  };
  // (device: window lists by a bitmap in LDS, devbuild.hpp dev_build_lw; AMGX_HOST_LW=1 keeps the host builder)
  const bool dev_lw = B.dev_images && !B.K.host_lw && !B.K.host_images;
  for (int g : values(DownLwLanes{})) {
    bool ok = false;
    if (dev_lw) {
      ok = dev_build_lw(B.csrA, false, g, B.K.lw_cap(LW_CAP), B.K.lw_test_cap_on, L.dinv.p, s.omega, L.ApreLW, L.lw_cptr, L.lw_ccol);
      if (ok && B.verify_images) verify_apre_lw(L, g, host_lw);
      if (!ok) { L.ApreLW = DevMatrix(); L.lw_cptr.release(); L.lw_ccol.release(); }
    }
    if (!ok) ok = host_lw(g, L.ApreLW, L.lw_cptr, L.lw_ccol);
    if (ok) { G = g; break; }
    L.ApreLW = DevMatrix();
  }
  if (!G) return false;
  L.fused_block = 512;
  build_restrict(B.K, s.P, L.RF, 512 / G, 4 * 512, 512);
  if (L.RF.empty()) { L.ApreLW = DevMatrix(); L.lw_cptr.release(); L.lw_ccol.release(); return false; }
  return true;
}

// levels whose A lies on at most 16 diagonals and equals its transpose bit for bit (Kuhn P1 matrices in natural vertex order):
// the fused down kernel streams the symmetric diagonal image of A instead of A' (dia_pre_restrict_kernel) -- 7 of the 15
// diagonals from HBM at cfg 2, the lower ones are shifted re-reads of the same arrays, and no index stream.  Not on levels
// a rank-partitioned driver runs stage by stage (dense_first < 0), nor below AMGX_DIA_MIN_ROWS rows (2 M: the smaller levels
// keep the SELL image), nor where the image would store more than AMGX_DIA_MAX_FILL (1.05) x the entries of A -- thin grids, whose
// boundary rows fill few of the diagonals.  AMGX_NO_DIA=1 disables it.
static bool dia_image(LevelBuild& B) {
  const amgx_level_desc& s = B.s;
  DevLevel& L = B.L;
  if (B.K.no_dia || B.dense_first < 0 || s.A.n_rows != s.A.n_cols || s.A.n_rows < std::max<int64_t>(1, B.K.dia_min_rows) ||
      s.omega == 0.0 || B.K.no_wdiag || !B.K.fused_restrict_ok(s.P, 1)) return false;
  // the kernel puts the diagonal term back as omega*b_i (0 where dinv_i = 0): dinv must be the plain inverse diagonal
  if (B.dev_images ? !B.diagA.plain : !host_diag_plain(s)) return false;
  auto par = [](int64_t nb, auto&& f) { par_for(nb, [&](int64_t a, int64_t b, int) { for (int64_t q = a; q < b; ++q) f(q); }, 1); };
  int32_t off[dia::MAX_UPPER];
  const int K = dia::detect(s.A.n_rows, s.A.n_cols, s.A.rowptr, s.A.col, s.A.val, dia::MAX_DIAGS, B.K.dia_max_fill, off, par);
  if (K <= 0 || K > DIA_MAX_UPPER) return false;
  DevDia& D = L.dia;
  D.K = K;
  for (int k = 0; k < K; ++k) D.off[k] = off[k];
  std::vector<double> hv;
  if (!B.dev_images || B.verify_images) {
    hv.resize((size_t)K * (size_t)s.A.n_rows);
    dia::upper_image(s.A.n_rows, s.A.rowptr, s.A.col, s.A.val, K, off, hv.data(), par);
  }
  if (B.dev_images) {
    dev_build_dia(B.csrA, D);
    if (B.verify_images) verify_dia(D, hv);
  } else
    D.val.upload(hv);
  L.fused_block = 512;
  // a lexicographic grid of at least AMGX_DIA_BOX_MIN_ROWS rows: box chunks (dia_box_pre_restrict_kernel); AMGX_NO_DIA_BOX=1 keeps
  // the chunks below, and so does every level grid_of / box_grid refuse or whose fullest box does not fit the kernel's LDS
  dia::Grid grid;
  dia::BoxGrid box;
  if (!B.K.no_dia_box && s.A.n_rows >= B.K.dia_box_min_rows && contains(DiaBoxDiags{}, K) && dia::grid_of(s.A.n_rows, K, off, grid) &&
      dia::box_grid(grid, K, B.K.dia_box_yc, B.K.dia_box_zc, box)) {
    const dia::BoxRuns runs = dia::box_runs(box);
    build_restrict(B.K, s.P, L.RF, box.box_rows(), DIA_BOX_LDS_DOUBLES - box.box_rows(), 512, nullptr, &runs);
    if (!L.RF.empty()) {
      L.RF.boxed = true;
      L.RF.box = box;
      L.RF.box_lds_doubles = box.box_rows() + std::max<int64_t>(box.box_rows(), L.RF.max_entries);
      // (more than 64 KB of dynamic LDS has to be allowed per kernel, once)
      auto allow = [&](auto KK) {
        HIPCHK(hipFuncSetAttribute((const void*)dia_box_pre_restrict_kernel<KK()>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                   DIA_BOX_LDS_DOUBLES * (int)sizeof(double)));
      };
      if (L.RF.box_lds_doubles * sizeof(double) > 65536) dispatch(DiaBoxDiags{}, K, allow);
      // ... and so has that of the multi-vector forms (AMGX_MULTI_FUSE_DOWN_DIA, sized by down_nv_dia_lds_bytes), for both widths:
      // here, at create time, because a call that carries the bit may be the one a stream capture records
      DownPlan nvp;
      nvp.family = DOWN_FAM_DIA_BOX; nvp.box_rows = box.box_rows(); nvp.max_entries = L.RF.max_entries;
      for (int nv : values(DownNvWidths{})) dispatch(DownNvWidths{}, nv, [&](auto NV) {
        const size_t bytes = down_nv_dia_lds_bytes(nvp, NV());
        if (bytes <= 65536 || bytes > DOWN_NV_DIA_LDS_MAX) return;
        dispatch(DiaBoxDiags{}, K, [&](auto KK) {
          HIPCHK(hipFuncSetAttribute((const void*)dia_box_pre_restrict_nv_kernel<KK(), NV()>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)DOWN_NV_DIA_LDS_MAX));
        });
      });
      return true;
    }
  }
  build_restrict_chunks(B.K, s.P, L.RF, 512, 6 * 512, 512, true);
  if (L.RF.empty()) { L.dia = DevDia(); return false; }
  return true;
}

// the chunk-local restriction for the image of A' the level got: the local-window image first, the SELL chunk form after it
static void fused_restrict(LevelBuild& B) {
  const amgx_level_desc& s = B.s;
  DevLevel& L = B.L;
  if (lw_image(B)) return;
  // fused pre-smoothing + restriction when A' is in the one-thread-per-row SELL form (big levels).
  // Same-process A/B with 4 instances per variant (profiles/r01/restrict_fused.txt): 1-3 % faster cycle than the
  // separate pre-smoothing + P^T gather kernels, and r is never written to HBM.  AMGX_NO_FUSED_RESTRICT=1 disables it.
  const int G = L.Apre.lanes;
  if (L.Apre.fmt == FMT_SELL && L.Apre.sell.win == SELL_WIN && G == 1 && SELL_WIN == 512 && B.K.fused_restrict_ok(s.P, 1))
  {
    L.fused_block = SELL_WIN;              // windowed A': a chunk = a window (sell_win_pre_restrict_kernel)
    build_restrict(B.K, s.P, L.RF, SELL_WIN, 6 * SELL_WIN, SELL_WIN);
  }
  else if (L.Apre.fmt == FMT_SELL && !L.Apre.sell.win && down_sell_lanes_ok(G) && B.K.fused_restrict_ok(s.P, G))
  {
    L.fused_block = B.K.fused_block;       // same-process A/B: 512 < 1024 (epilogues of more, smaller workgroups overlap better)
    if (G > 1) L.fused_block = 512;        // (several lanes per row: the chunk holds 512 / G rows)
    // big square one-thread-per-row levels: compact chunks (cluster_slices) -- fewer partial sums per coarse row
    // (not on a handle that a rank-partitioned driver runs stage by stage -- dense_first < 0 --: its launches cover interior and
    //  boundary chunk RANGES, which only consecutive chunks have; a rank without ghost columns, e.g. world size 1, has a square level)
    build_restrict_chunks(B.K, s.P, L.RF, L.fused_block / G, 6 * L.fused_block, L.fused_block, G == 1 && B.dense_first >= 0 && s.A.n_rows == s.A.n_cols);
    // several lanes per row: the kernel exists for 4 entries of P per thread only; a chunk of 512 / G rows with more
    // than 2048 entries (a prolongation with more than 4 G entries per row) keeps the separate kernels
    if (G > 1 && L.RF.ept != DOWN_MULTI_EPT) L.RF = DevRestrict();
  }
}

// task "A' + fused restriction": the diagonal image, else A' on the device, else A' on the host; then the chunk-local restriction
static void jacobi_down_task(LevelBuild& B) {
  const amgx_level_desc& s = B.s;
  DevLevel& L = B.L;
  if (dia_image(B)) return;
  // (device builder: A' = A diag(omega Dinv) from the CSR of A that is already there; the diagonal slot carries omega*Dinv_i
  //  under the same conditions as below)
  const bool dev_wdiag = s.omega != 0.0 && !B.K.no_wdiag && B.diagA.plain;
  // levels >= 1 of a reference-shaped hierarchy have ragged long rows (plain slices pad 20 % at the 1.24 M-row level of cfg 2,
  // length-sorted windows 3.6 %).  Measured NON-win (profiles/r04/l1_experiments.txt): the windowed image with its fused kernel
  // (sell_win_pre_restrict_kernel) runs that level in 256 us against 215 us -- these levels are bound by the scattered gathers
  // of x, and sorting the rows of a window by length puts unrelated rows into neighbouring lanes.  Opt-in: AMGX_APRE_WINDOW=1.
  const int apre_win = (B.l >= 1 && s.A.n_rows == s.A.n_cols && B.K.apre_window) ? SELL_WIN : 0;
  if (B.dev_images && !B.verify_images &&
      dev_upload_matrix(B.K, B.csrA, L.Apre, true, 1.35, apre_win, &B.diagA, L.dinv.p, s.omega, dev_wdiag ? L.dinv.p : nullptr)) {
    fused_restrict(B);
    return;
  }
  // column-scaled image for the fused pre-smoothing pass (memory for bandwidth: one more copy of A)
  const std::unique_ptr<double[]> sv = scaled_values(s);
  amgx_matrix As = s.A;
  As.val = sv.get();
  // one-thread-per-row form: the diagonal slot carries omega*Dinv_i (SellMat::wdiag), the epilogue then needs no
  // dinv stream (80 MB per pass at cfg 2); AMGX_NO_WDIAG=1 keeps A'_ii there
  std::vector<double> wdv;
  if (s.omega != 0.0 && !B.K.no_wdiag) {
    // the epilogue re-inserts A'_ii b_i as omega*b_i (or 0 where dinv_i = 0): valid iff dinv is the plain inverse diagonal
    if (host_diag_plain(s)) {
      wdv.resize((size_t)s.A.n_rows);
      par_for(s.A.n_rows, [&](int64_t i0, int64_t i1, int) { for (int64_t i = i0; i < i1; ++i) wdv[i] = s.omega * s.dinv[i]; }, 1 << 16);
    }
  }
  const double* wd = wdv.empty() ? nullptr : wdv.data();
  if (B.dev_images && B.verify_images) verify_build_apre(B.K, As, B.csrA, B.diagA, s.omega, apre_win, wd, dev_wdiag, L);
  else upload_matrix(B.K, As, L.Apre, "A (pre-smoothing image)", true, true, false, 1.35, apre_win, wd);
  fused_restrict(B);
}

static void build_jacobi_down(LevelBuild& B, SetupTasks& tasks) {
  tasks.run([&B] { jacobi_down_task(B); }, "A' + fused restriction");
}

// ---- post-smoothing folded into the prolongation (V-cycle) -----------------------------------------------------------------

// the local-window image of a Q that the device product left in csrQ: device builder, else the host builder from a download
static void build_qlw_of_dev_q(LevelBuild& B, const DevCsrSrc& csrQ) {
  const amgx_level_desc& s = B.s;
  DevLevel& L = B.L;
  bool qlw_done = false;
  if (!B.K.host_lw) {
    qlw_done = dev_build_lw(csrQ, true, 1, B.K.lw_cap_small(QW_CAP), B.K.lw_test_cap_on, nullptr, 0.0, L.QLW, L.qlw_cptr, L.qlw_ccol);
    if (!qlw_done) { L.QLW = DevMatrix(); L.qlw_cptr.release(); L.qlw_ccol.release(); }
    else if (B.verify_images) verify_qlw(B.K, csrQ, s.A.n_rows, L);
  }
  if (!qlw_done) {
    SetupClock qclk(B.K);
    std::vector<int64_t> rp = db_download(csrQ.rowptr, (size_t)s.A.n_rows + 1);
    std::vector<int32_t> cc = db_download(csrQ.col, (size_t)std::max<int64_t>(1, csrQ.nnz));
    std::vector<double> vv = db_download(csrQ.val, (size_t)std::max<int64_t>(1, csrQ.nnz));
    qclk.lap("  lw-win: download of Q", B.l);
    if (!build_sell_lw_windowed(B.K, s.A.n_rows, csrQ.n_cols, rp.data(), cc.data(), vv.data(), L.QLW, L.qlw_cptr, L.qlw_ccol)) L.QLW = DevMatrix();
  }
}

// task "Q = (I - w Dinv A) P" on a square scalar level: the sparse product and the windowed image of its result on the device
// (devbuild.hpp), else on the host
static void scalar_q_task(LevelBuild& B) {
  const amgx_level_desc& s = B.s;
  DevLevel& L = B.L;
  const double qpad = B.K.q_max_pad;
  if (B.dev_images) {
    check_matrix(s.P, "P");
    DevCsrSrc csrP, csrQ;
    csrP.upload(s.P);
    if (dev_fold_prolongation(B.csrA, csrP, L.dinv.p, s.omega, csrQ) && dev_upload_matrix(B.K, csrQ, L.Q, false, qpad, SELL_WIN, nullptr)) {
      if (B.K.qlw_wanted(s.A.n_rows)) build_qlw_of_dev_q(B, csrQ);
      if (B.verify_images) verify_q(B.K, s, csrQ, qpad, L.Q);
      return;
    }
    L.Q = DevMatrix();
    if (B.verify_images) std::fprintf(stderr, "[amgx_create] AMGX_VERIFY_IMAGES: level %d: Q is left to the host builder\n", B.l);
  }
  HostCsr q;
  fold_prolongation(s.A, s.P, s.dinv, s.omega, q);
  if (q.rowptr[s.A.n_rows] < I32_MAX) {
    amgx_matrix Qm = s.P;
    Qm.rowptr = q.rowptr.data(); Qm.col = q.col.data(); Qm.val = q.val.data();
    upload_matrix(B.K, Qm, L.Q, "Q (folded post-smoothing prolongation)", true, false, false, qpad, SELL_WIN);
    if (B.K.qlw_wanted(s.A.n_rows) &&
        !build_sell_lw_windowed(B.K, s.A.n_rows, s.P.n_cols, q.rowptr.data(), q.col.data(), q.val.data(), L.QLW, L.qlw_cptr, L.qlw_ccol)) L.QLW = DevMatrix();
  }
}

// block Jacobi levels of the V-cycle: the same fold in block form (Q has the block shape of P)
static void block_q_task(LevelBuild& B) {
  const amgx_level_desc& s = B.s;
  DevLevel& L = B.L;
  HostCsr q;
  fold_prolongation(s.A, s.P, s.dinv, s.omega, q);
  // Fold only where it pays: the way up then streams Q instead of A + P (+ the round trip of x + P x_c), but
  // rectangular-block Q runs through the CSR block kernels (~4.5 TB/s) while square-block A streams as BSELL
  // (~6.5 TB/s).  Measured at the cfg 3 shapes (profiles/r01/block_fold.txt): 3x3 fine level with 3x6 blocks in
  // P: Q has 10.8 blocks/row = 1.6 GB vs A + P = 1.65 GB -> literal is 55 us faster; 6x6 levels: Q = 0.36 GB
  // vs 1.04 GB -> folded is 100 us faster.
  auto bytes = [](int64_t nnz, int br, int bc) { return (double)nnz * (8.0 * br * bc + 4.0); };
  const double bq = bytes(q.rowptr[s.A.n_rows], s.P.br, s.P.bc);
  const double blit = bytes(s.A.rowptr[s.A.n_rows], s.A.br, s.A.bc) + bytes(s.P.rowptr[s.P.n_rows], s.P.br, s.P.bc);
  if (q.rowptr[s.A.n_rows] < I32_MAX && bq < 0.7 * blit) {
    amgx_matrix Qm = s.P;
    Qm.rowptr = q.rowptr.data(); Qm.col = q.col.data(); Qm.val = q.val.data();
    upload_matrix(B.K, Qm, L.Q, "Q (folded post-smoothing prolongation)");
  }
}

// Square levels: Q is built here.  Rank-partitioned levels: Q needs the P rows of the ghost vertices, so the caller supplies it
// (amgx_level_desc.Q) and drives the level through amgx_cycle_down / amgx_cycle_up.
static void build_folded_prolongation(LevelBuild& B, SetupTasks& tasks) {
  const amgx_level_desc &s = B.s, &c = *B.c;
  const bool one_step = s.sm_type == AMGX_SM_JACOBI && s.sm_steps <= 1 && !s.sm_symm;
  if (one_step && s.A.br == 1 && B.cycle == AMGX_CYCLE_V && s.P.br == 1 && s.P.bc == 1 && !B.K.no_fold) {
    if (s.Q.rowptr) {
      if (s.Q.n_rows != s.A.n_rows || s.Q.br != 1 || s.Q.bc != 1 || s.Q.n_cols < c.A.n_rows || s.Q.n_cols > c.A.n_cols)
        throw Err("Q does not match the level matrices");
      if (s.Q.rowptr[s.Q.n_rows] >= I32_MAX) throw Err("Q: too many entries");
      tasks.run([&B] {
        const amgx_level_desc& s = B.s;
        DevLevel& L = B.L;
        upload_matrix(B.K, s.Q, L.Q, "Q (folded post-smoothing prolongation)", true, false, false, B.K.q_max_pad, SELL_WIN);
        // (rank-partitioned level: the caller's Q, columns [owned | ghost] of the coarse level)
        if (B.K.qlw_wanted(s.A.n_rows) &&
            !build_sell_lw_windowed(B.K, s.Q.n_rows, s.Q.n_cols, s.Q.rowptr, s.Q.col, s.Q.val, L.QLW, L.qlw_cptr, L.qlw_ccol)) L.QLW = DevMatrix();
      });
    } else if (s.A.n_rows == s.A.n_cols && s.P.n_cols == c.A.n_rows)
      tasks.run([&B] { scalar_q_task(B); }, "Q = (I - w Dinv A) P");
  }
  if (one_step && s.A.br > 1 && B.cycle == AMGX_CYCLE_V && s.A.n_rows == s.A.n_cols && s.P.n_cols == c.A.n_rows && s.P.br == s.A.br &&
      !B.K.no_fold && !B.K.no_block_fold)
    tasks.run([&B] { block_q_task(B); });
}

// scalar Chebyshev levels: the residual after pre-smoothing feeds the chunk-local restriction without going through HBM
// (sell_pre_restrict_kernel<.., MODE 2> on the SELL image of A itself), under the rule of the Jacobi levels' fused down kernel.
// AMGX_CHEB_NO_FUSED_RESTRICT=1 (or AMGX_NO_FUSED_RESTRICT=1) keeps EP_RES + the separate restriction kernels.
static void cheb_fused_restrict(LevelBuild& B) {
  const amgx_level_desc& s = B.s;
  DevLevel& L = B.L;
  if (s.sm_type == AMGX_SM_CHEBY && s.A.br == 1 && s.sm_steps <= 1 && !s.sm_symm && L.A.fmt == FMT_SELL && !L.A.sell.win &&
      down_sell_lanes_ok(L.A.lanes) && B.K.fused_restrict_ok(s.P, L.A.lanes) &&
      !B.K.cheb_no_fused_restrict)
  {
    const int G = L.A.lanes;
    L.fused_block = 512;
    build_restrict_chunks(B.K, s.P, L.RF, 512 / G, 6 * 512, 512, G == 1 && B.dense_first >= 0);
    if (G > 1 && L.RF.ept != DOWN_MULTI_EPT) L.RF = DevRestrict();
  }
}

// Levels with mat_prec = AMGX_PREC_F32: the single-precision images -- the value array of an image rounded to
// float on the device, every index array shared.  Which levels and which images get one is decided HERE and nowhere else:
//   Chebyshev levels: A in plain sliced-ELL (any lanes per row) or BSELL (2x2, 3x3, 6x6) -- the formats of the levels that carry bytes;
//     CSR-vector, windowed SELL and block CSR levels (small / irregular) stay fp64 silently.  From here on every smoother pass of the
//     level (the EP_CHEB steps, update_res, the residual before the restriction incl. its fused form) reads it.
//   Gauss-Seidel levels whose sweep form is hybrid-block, block-coloured or multicolour BSELL (SWEEP_BGSB, SWEEP_BGSB_BC,
//     SWEEP_MC_BSELL; 2x2, 3x3, 6x6): every BSELL image the level has of bgsb.off / in / upin / rest / offlo or gs.bcopy / blower /
//     bupper, and A itself where it is BSELL (an A that stayed in block CSR -- a small level -- gets its rounded values at fp64
//     width, DevMatrix::val64r, so that sweeps and residual see one operator).  The sweeps and the residual after the sweep from zero
//     (its split identities and the unsplit product with A) read them (DevLevel::gs32); update_res of a general sweep reads the
//     fp64 A (Handle::base_smooth says why).  Every other Gauss-Seidel form (scalar levels, the row list over block CSR) stays
//     fp64 silently.  No class of images is excluded: see DESIGN.md 6 for what was measured and what was not.
//     AMGX_GS_F32_WIDE=1 (A/B twin): no float images; the rounded values are written back into the fp64 arrays of exactly these
//     images (A: into DevMatrix::val64r, its true values stay) and the fp64 kernels run -- same bits, fp64 bytes.
// amgx_matvec, amgx_residual, the Krylov operator and the lambda_max estimate keep the fp64 image of A.
// A value that rounds to +-inf is an error that names the level; nothing half-built is left behind.
// AMGX_NO_MAT_F32=1 ignores every request (the handle is then the double handle, bit for bit).
//   Scalar Gauss-Seidel levels with mat_prec = AMGX_PREC_F32_SCALAR_GS: scalar_gs_f32_images below.
static void jacobi_f32_images(LevelBuild& B);
static void scalar_gs_f32_images(LevelBuild& B);
static void mat_f32_image(LevelBuild& B) {
  const amgx_level_desc& s = B.s;
  DevLevel& L = B.L;
  if (B.smoothed() && s.jacobi_prec != AMGX_JACOBI_PREC_F64 && !B.K.no_mat_f32) jacobi_f32_images(B);
  if (B.smoothed() && s.mat_prec == AMGX_PREC_F32_SCALAR_GS && !B.K.no_mat_f32) scalar_gs_f32_images(B);
  if (!B.smoothed() || s.mat_prec != AMGX_PREC_F32 || B.K.no_mat_f32) return;
  auto beyond = [&](int64_t bad, const char* what) {
    return Err("amgx_create: level " + std::to_string(B.l) + ": " + std::to_string(bad) + " value(s) of " + what +
               " are beyond the range of single precision (mat_prec = AMGX_PREC_F32)");
  };
  if (s.sm_type == AMGX_SM_CHEBY) {
    const bool sell = L.A.fmt == FMT_SELL && !L.A.sell.win;
    const bool bsell = L.A.fmt == FMT_BSELL && (L.A.br == 2 || L.A.br == 3 || L.A.br == 6);
    if (!sell && !bsell) return;
    const int64_t bad = dev_round_to_f32(sell ? L.A.sell.val : L.A.bsell.val, L.A.val32);
    if (bad) {
      L.A.val32.release();
      throw beyond(bad, "A");
    }
    return;
  }
  if (s.sm_type != AMGX_SM_GS || (L.bs != 2 && L.bs != 3 && L.bs != 6)) return;
  const int form = sweep_path(L);
  if (form != SWEEP_BGSB && form != SWEEP_BGSB_BC && form != SWEEP_MC_BSELL) return;
  // the images the level's form reads (an image the level does not have is empty: no slices, no values)
  std::vector<DevMatrix*> sweep_only;
  if (form == SWEEP_MC_BSELL) sweep_only = {&L.gs.bcopy, &L.gs.blower, &L.gs.bupper};
  else sweep_only = {&L.bgsb.off, &L.bgsb.in, &L.bgsb.upin, &L.bgsb.rest, &L.bgsb.offlo};
  const bool wide = B.K.gs_f32_wide;
  auto undo = [&] {
    for (DevMatrix* M : sweep_only) M->val32.release();
    L.A.val32.release(); L.A.val64r.release();
    L.gs32 = L.gs32_wide = false; L.gs32_images = 0; L.gs32_bytes = 0;
  };
  // (the range check comes first, on A: every image holds values of A or, in `rest`, diagonal blocks scaled by a factor in [0, 1].
  // The wide twin overwrites the sweep images, so it must not start before the level is known to be representable)
  auto one = [&](DevMatrix& M, const char* what, bool keep64) {
    if (keep64 && M.fmt == FMT_CSRVEC && M.br > 1 && M.val.n > 0) {        // A in block CSR: rounded values at fp64 width, no float image
      const int64_t bad = dev_round_to_f32_wide(M.val, M.val64r);
      if (bad) { undo(); throw beyond(bad, what); }
      return;
    }
    if (M.fmt != FMT_BSELL || M.bsell.val.n == 0) return;
    int64_t bad;
    if (!wide) bad = dev_round_to_f32(M.bsell.val, M.val32);
    else if (keep64) bad = dev_round_to_f32_wide(M.bsell.val, M.val64r);
    else bad = dev_round_to_f32_wide(M.bsell.val, M.bsell.val);
    if (bad) { undo(); throw beyond(bad, what); }
    L.gs32_images += 1;
    L.gs32_bytes += (wide ? 8 : 4) * (int64_t)M.bsell.val.n;
  };
  if (wide) {                     // a dry run on the values of A decides before anything is overwritten
    DevBuf<float> probe;
    const DevBuf<double>& av = L.A.fmt == FMT_BSELL ? L.A.bsell.val : L.A.val;
    const int64_t bad = dev_round_to_f32(av, probe);
    if (bad) throw beyond(bad, "A");
  }
  one(L.A, "A", true);
  static const char* names_mc[] = {"the colour-major copy of A", "its lower part", "its upper part"};
  static const char* names_hb[] = {"the image `off`", "the image `in`", "the image `upin`", "the image `rest`", "the image `offlo`"};
  for (size_t i = 0; i < sweep_only.size(); ++i) one(*sweep_only[i], form == SWEEP_MC_BSELL ? names_mc[i] : names_hb[i], false);
  (wide ? L.gs32_wide : L.gs32) = true;
}

// Scalar Jacobi levels with jacobi_prec != 0 (check_level has refused every other level).  The images are rounded AS
// STORED: A' holds a_ij * omega * dinv_j (its diagonal slot omega * dinv_i under wdiag), Q holds (I - omega Dinv A) P.  Converted, where
// the level has them: A, A', Q in plain sliced-ELL, the local-window images of A' and Q, the symmetric diagonal image.  CSR-vector and
// windowed sliced-ELL images, P, P^T, the restriction data, dinv, the tail program's copies and the dense tail stay fp64.
//   AMGX_JACOBI_PREC_F32: a float value array per image (DevMatrix::val32, DevDia::val32); the fp64 values of every image but A are
//     released -- only the Jacobi passes read them, and those read the float array from here on.  A keeps both: update_res,
//     amgx_matvec, amgx_residual and the Krylov operator read the fp64 one.
//   AMGX_JACOBI_PREC_F32_WIDE: the rounded values at fp64 width, in place (A: DevMatrix::val64r); the fp64 kernels run.
// Range check first, on every image, before anything is overwritten or released; a value beyond float is an error that names the level.
static void jacobi_f32_images(LevelBuild& B) {
  const amgx_level_desc& s = B.s;
  DevLevel& L = B.L;
  const bool wide = s.jacobi_prec == AMGX_JACOBI_PREC_F32_WIDE;
  auto plain_sell = [](const DevMatrix& M) { return !M.empty() && M.fmt == FMT_SELL && !M.sell.win && M.sell.val.n > 0; };
  // the local-window forms: A' in plain slices with window columns, Q windowed with window columns -- sliced-ELL value arrays both
  auto lw_sell = [](const DevMatrix& M) { return !M.empty() && M.fmt == FMT_SELL && M.sell.val.n > 0; };
  struct Img { DevMatrix* M; int bit; const char* what; bool keep64; };
  std::vector<Img> imgs;
  if (plain_sell(L.A)) imgs.push_back({&L.A, 0, "A", true});
  if (plain_sell(L.Apre)) imgs.push_back({&L.Apre, 1, "A'", false});
  if (lw_sell(L.ApreLW)) imgs.push_back({&L.ApreLW, 2, "the local-window image of A'", false});
  if (plain_sell(L.Q)) imgs.push_back({&L.Q, 4, "Q", false});
  if (lw_sell(L.QLW)) imgs.push_back({&L.QLW, 5, "the local-window image of Q", false});
  const bool dia = L.dia.on() && L.dia.val.n > 0;
  auto beyond = [&](int64_t bad, const char* what) {
    return Err("amgx_create: level " + std::to_string(B.l) + ": " + std::to_string(bad) + " value(s) of " + what +
               " are beyond the range of single precision (jacobi_prec = " + (wide ? "AMGX_JACOBI_PREC_F32_WIDE" : "AMGX_JACOBI_PREC_F32") + ")");
  };
  auto undo = [&] {
    for (const Img& im : imgs) { im.M->val32.release(); im.M->val64r.release(); }
    L.dia.val32.release();
    L.jp32 = L.jp32_wide = false; L.jp_mask = 0; L.jp_bytes = L.jp_released = 0;
  };
  // pass 1: the float arrays (the wide twin drops them again: its dry run)
  for (const Img& im : imgs) {
    const int64_t bad = dev_round_to_f32(im.M->sell.val, im.M->val32);
    if (bad) { undo(); throw beyond(bad, im.what); }
    if (wide) im.M->val32.release();
  }
  if (dia) {
    const int64_t bad = dev_round_to_f32(L.dia.val, L.dia.val32);
    if (bad) { undo(); throw beyond(bad, "the diagonal image"); }
    if (wide) L.dia.val32.release();
  }
  // pass 2: nothing can fail for range any more
  for (const Img& im : imgs) {
    const int64_t n = (int64_t)im.M->sell.val.n;
    if (wide) {
      if (im.keep64) dev_round_to_f32_wide(im.M->sell.val, im.M->val64r);
      else dev_round_to_f32_wide(im.M->sell.val, im.M->sell.val);
    } else if (!im.keep64) {
      im.M->sell.val.release();
      L.jp_released += 8 * n;
    }
    L.jp_mask |= 1 << im.bit;
    L.jp_bytes += (wide ? 8 : 4) * n;
  }
  if (dia) {
    const int64_t n = (int64_t)L.dia.val.n;
    if (wide) dev_round_to_f32_wide(L.dia.val, L.dia.val);
    else {
      L.dia.val.release();
      L.jp_released += 8 * n;
      // (the float box kernel takes the same dynamic LDS as the fp64 one: more than 64 KB has to be allowed per kernel, once)
      if (L.RF.boxed && L.RF.box_lds_doubles * sizeof(double) > 65536)
        dispatch(DiaBoxDiags{}, L.dia.K, [&](auto KK) {
          HIPCHK(hipFuncSetAttribute((const void*)dia_box_pre_restrict_kernel<KK(), float>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     DIA_BOX_LDS_DOUBLES * (int)sizeof(double)));
        });
    }
    L.jp_mask |= 1 << 3;
    L.jp_bytes += (wide ? 8 : 4) * n;
  }
  if (L.jp_mask) (wide ? L.jp32_wide : L.jp32) = true;
}

// The multi-vector form of the local-window down launch (AMGX_MULTI_FUSE_DOWN_F32, sized by down_nv_lw_lds_bytes) holds the window of
// the longest list for NV columns: more than 64 KB of dynamic LDS has to be allowed per kernel, once -- here, at create time, because a
// call that carries the bit may be the one a stream capture records.  For both widths, for the value type the launch reads.
static void allow_down_nv_lw(const DevLevel& L) {
  const DownPlan& p = L.plan_rg;
  if (!p.on || p.family != DOWN_FAM_LW) return;
  for (int nv : values(DownNvWidths{})) dispatch(DownNvWidths{}, nv, [&](auto NV) {
    if (!down_nv_lw_ok(p, NV()) || down_nv_lw_lds_bytes(p, NV()) <= 65536) return;
    dispatch(DownLwLanes{}, p.lanes, [&](auto G) { dispatch(DownLwEpt{}, p.ept, [&](auto EPT) {
      if (p.f32) HIPCHK(hipFuncSetAttribute((const void*)sell_lw_pre_restrict_nv_kernel<EPT(), G(), 1, NV(), float>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)DOWN_NV_DIA_LDS_MAX));
      else HIPCHK(hipFuncSetAttribute((const void*)sell_lw_pre_restrict_nv_kernel<EPT(), G(), 1, NV(), double>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)DOWN_NV_DIA_LDS_MAX));
    }); });
  });
}

// Scalar Gauss-Seidel levels with mat_prec = AMGX_PREC_F32_SCALAR_GS (check_level has refused every other level).  Each
// sweep image the level's form has -- block-hybrid: gsb.full, fullLW, lowin, rest, restLW; multicolour: gs.sell, lower, upper -- gets a
// float value array, the stored fp64 values rounded to nearest; index arrays, rowid, slotcolor and the window lists are shared.  dinv,
// gsb.cvec, the vectors, P, P^T, the restriction data, the tail program's copies and the dense tail stay fp64 and true.
//   A gets an image only on a level WITHOUT split images, where residual_after_zero reads A (residual_sm): a float array where A is
//   plain sliced-ELL, else -- a format without a float kernel -- the rounded values at fp64 width in DevMatrix::val64r.  A keeps its
//   true fp64 values for update_res, amgx_matvec, amgx_residual and the Krylov operator.  `rest` in CSR-vector form (a badly padded
//   remainder: a small level) has no float kernel either: its values are rounded in place at fp64 width.
//   The fp64 value arrays of the sweep images are released: only the sweeps and the residual after the sweep from zero read them, and
//   those read the float arrays from here on (Handle::sgs_image and Handle::product refuse an fp64 view of a released image).
//   AMGX_GS_F32_WIDE=1 (A/B twin): no float arrays; the rounded values at fp64 width, in place (A: val64r); the fp64 kernels run.
// Range check first, on every image, before anything is overwritten or released; a value beyond float is an error that names the level.
static void scalar_gs_f32_images(LevelBuild& B) {
  DevLevel& L = B.L;
  const int form = sweep_path(L);
  if (form != SWEEP_GSB && form != SWEEP_MC) return;       // (a level without rows or without a colouring: nothing to convert)
  const bool wide = B.K.gs_f32_wide;
  // val: the fp64 values; v32: where the float array goes (null: no float kernel for the format); v64r / keep64: A keeps its true values
  struct Img { DevBuf<double>* val; DevBuf<float>* v32; DevBuf<double>* v64r; int bit; const char* what; bool keep64; };
  std::vector<Img> imgs;
  auto sell_img = [&](DevMatrix::Sell& S, int bit, const char* what) { if (S.val.n > 0) imgs.push_back({&S.val, &S.val32, nullptr, bit, what, false}); };
  auto mat_img = [&](DevMatrix& M, int bit, const char* what) {
    if (M.empty()) return;
    if (M.fmt == FMT_SELL) { if (M.sell.val.n > 0) imgs.push_back({&M.sell.val, &M.val32, nullptr, bit, what, false}); }
    else if (M.fmt == FMT_CSRVEC && M.br == 1 && M.val.n > 0) imgs.push_back({&M.val, nullptr, nullptr, bit, what, false});
  };
  bool split = false;
  if (form == SWEEP_GSB) {
    DevGSB& g = L.gsb;
    split = g.has_split;
    sell_img(g.full, 1, "the image `full`");
    if (g.has_fullLW) sell_img(g.fullLW, 2, "the local-window image of `full`");
    if (split) {
      sell_img(g.lowin, 3, "the image `lowin`");
      mat_img(g.rest, 4, "the image `rest`");
      mat_img(g.restLW, 5, "the local-window image of `rest`");
    }
  } else {
    DevGS& g = L.gs;
    split = g.has_split;
    sell_img(g.sell, 6, "the colour-major copy of A");
    if (split) { sell_img(g.lower, 7, "its lower part"); sell_img(g.upper, 8, "its upper part"); }
  }
  if (!split && !L.A.empty()) {
    const bool plain_sell = L.A.fmt == FMT_SELL && !L.A.sell.win;
    DevBuf<double>* av = L.A.fmt == FMT_SELL ? &L.A.sell.val : (L.A.fmt == FMT_CSRVEC && L.A.br == 1 ? &L.A.val : nullptr);
    if (av && av->n > 0) imgs.push_back({av, plain_sell ? &L.A.val32 : nullptr, &L.A.val64r, 0, "A", true});
  }
  auto beyond = [&](int64_t bad, const char* what) {
    return Err("amgx_create: level " + std::to_string(B.l) + ": " + std::to_string(bad) + " value(s) of " + what +
               " are beyond the range of single precision (mat_prec = AMGX_PREC_F32_SCALAR_GS)");
  };
  auto undo = [&] {
    for (const Img& im : imgs) { if (im.v32) im.v32->release(); if (im.v64r) im.v64r->release(); }
    L.sgs32 = L.sgs32_wide = false; L.sgs_mask = 0; L.sgs_bytes = L.sgs_released = 0;
  };
  // pass 1: the float arrays; an image that gets none (the twin; a format without a float kernel) drops its array again: a dry run
  for (const Img& im : imgs) {
    DevBuf<float> probe;
    DevBuf<float>& dst = im.v32 ? *im.v32 : probe;
    const int64_t bad = dev_round_to_f32(*im.val, dst);
    if (bad) { undo(); throw beyond(bad, im.what); }
    if (wide) dst.release();
  }
  // pass 2: nothing can fail for range any more
  for (const Img& im : imgs) {
    const int64_t n = (int64_t)im.val->n;
    const bool f32 = !wide && im.v32;
    if (im.keep64) { if (!f32) dev_round_to_f32_wide(*im.val, *im.v64r); }          // A: the true values stay
    else if (!f32) dev_round_to_f32_wide(*im.val, *im.val);                          // the twin, or `rest` in CSR-vector form: in place
    else { im.val->release(); L.sgs_released += 8 * n; }
    L.sgs_mask |= 1 << im.bit;
    L.sgs_bytes += (f32 ? 4 : 8) * n;
  }
  if (L.sgs_mask) (wide ? L.sgs32_wide : L.sgs32) = true;
}

// workgroup -> rows mapping of the streaming kernels on this level (SellMat::xcd)
static void set_xcd_modes(LevelBuild& B) {
  const amgx_level_desc& s = B.s;
  DevLevel& L = B.L;
  const int mode = B.K.xcd;
  const double avg = s.A.n_rows ? (double)s.A.rowptr[s.A.n_rows] / (double)s.A.n_rows : 0.0;
  const int on = mode >= 2 || (mode == 1 && avg >= 24.0 && s.A.n_rows >= 200000);
  L.A.sell.xcd = L.Apre.sell.xcd = L.Q.sell.xcd = L.gsb.rest.sell.xcd = on;
  L.dia.xcd = B.K.dia_xcd ? 1 : 0;        // (A/B hook: each XCD walks one contiguous eighth of the chunks)
  if (mode >= 3) L.P.sell.xcd = L.PT.sell.xcd = on;
}

static void alloc_level_vectors(LevelBuild& B) {
  DevLevel& L = B.L;
  const size_t len = (size_t)std::max<int64_t>(1, L.ext_len());
  L.x.alloc(len); L.rhs.alloc(len); L.res.alloc(len); L.tmp.alloc(len);
  HIPCHK(hipMemset(L.x.p, 0, len * sizeof(double)));
  HIPCHK(hipMemset(L.rhs.p, 0, len * sizeof(double)));
  HIPCHK(hipMemset(L.res.p, 0, len * sizeof(double)));
  HIPCHK(hipMemset(L.tmp.p, 0, len * sizeof(double)));
  if (L.sm_type == AMGX_SM_CHEBY) { L.d.alloc(len); HIPCHK(hipMemset(L.d.p, 0, len * sizeof(double))); }
}

// ---- after the level loop ---------------------------------------------------------------------------------------------------

// clev = inv: the inverse handed over by the host, or the coarsest matrix inverted on its free dofs here
static void build_coarse_inverse(Handle& h, const amgx_hierarchy_desc* d, const amgx_level_desc& s) {
  const DevLevel& L = h.lev.back();
  if (d->coarse_n != L.len()) throw Err("clev = inv: coarse_n does not match the coarsest level");
  h.coarse_n = d->coarse_n;
  if (d->coarse_inv) {
    h.coarse_ld = d->coarse_n;
    h.coarse_inv.upload(d->coarse_inv, (size_t)d->coarse_n * d->coarse_n);
    return;
  }
  // no inverse handed over (the host setup stops at 4096 unknowns): invert the coarsest matrix on its free dofs here
  // (dense_spd.hpp: blocked Gauss-Jordan, trailing updates on the matrix cores)
  const int64_t cap = h.knobs.coarse_dense_max;
  if (s.A.n_rows != s.A.n_cols) throw Err("clev = inv: the coarsest level of a rank-partitioned hierarchy cannot be inverted locally");
  if (d->coarse_n > cap) throw Err("clev = inv: coarsest level has " + std::to_string(d->coarse_n) + " unknowns, more than AMGX_COARSE_DENSE_MAX = " +
                                   std::to_string(cap) + " (a dense inverse would stream " + std::to_string(8 * d->coarse_n * d->coarse_n / 1000000) + " MB per application)");
  const int64_t n = d->coarse_n, npad = (n + GJ_T - 1) / GJ_T * GJ_T;
  const int bs = s.A.br;
  struct { DevBuf<int32_t> rowptr, col; DevBuf<double> val; } cA;       // (DevCsr holds scalar matrices only)
  {
    const int64_t nnzc = s.A.rowptr[s.A.n_rows];
    std::vector<int32_t> rp((size_t)s.A.n_rows + 1);
    for (int64_t i = 0; i <= s.A.n_rows; ++i) rp[i] = (int32_t)s.A.rowptr[i];
    cA.rowptr.upload(rp);
    cA.col.upload(s.A.col, (size_t)nnzc);
    cA.val.upload(s.A.val, (size_t)nnzc * bs * bs);
  }
  DevBuf<uint8_t> fr;
  if (s.free_dofs) fr.upload(s.free_dofs, (size_t)s.A.n_rows);
  h.coarse_inv.alloc((size_t)npad * npad);
  h.coarse_ld = npad;
  launch(gj_zero_kernel, Handle::grid_for(npad * npad), BLOCK, 0, h.stream, npad * npad, h.coarse_inv.p);
  launch(gj_scatter_kernel, Handle::grid_for(s.A.n_rows), BLOCK, 0, h.stream, s.A.n_rows, bs, cA.rowptr.p, cA.col.p, cA.val.p,
                     fr.p, npad, h.coarse_inv.p);
  launch(gj_fix_diag_kernel, Handle::grid_for(npad), BLOCK, 0, h.stream, npad, n, bs, fr.p, npad, 1.0, h.coarse_inv.p);
  h.coarse_pivot = dense_spd_inverse(h.coarse_inv.p, npad, npad, h.stream);
  if (!(h.coarse_pivot > 1e-14)) throw Err("clev = inv: the coarsest matrix is not positive definite on its free dofs (pivot ratio " +
                                           std::to_string(h.coarse_pivot) + "); use clev = none or a smaller coarsest level");
  launch(gj_fix_diag_kernel, Handle::grid_for(npad), BLOCK, 0, h.stream, npad, n, bs, fr.p, npad, 0.0, h.coarse_inv.p);
  HIPCHK(hipStreamSynchronize(h.stream));
}

// first level of the single-workgroup coarse tail (V-cycle, plain scalar smoothers, exact coarse solve, square levels); -1: none
static int tail_first_level(const Handle& h, const amgx_hierarchy_desc* d, const amgx_level_desc* levels) {
  const int L = d->n_levels;
  if (!(d->cycle == AMGX_CYCLE_V && d->clev == AMGX_CLEV_INV && L >= 2 && !h.knobs.no_tail_kernel)) return -1;
  int T = L - 1;
  while (T - 1 >= 1) {
    const amgx_level_desc& s = levels[T - 1];
    const int64_t cap = s.sm_type == AMGX_SM_GS ? TAIL_MAX_ROWS_GS : TAIL_MAX_ROWS;
    const bool ok = s.A.br == 1 && s.A.n_rows == s.A.n_cols && s.A.n_rows <= cap &&
                    (s.sm_type == AMGX_SM_JACOBI || (s.sm_type == AMGX_SM_GS && s.color && s.n_colors > 0 && s.gs_block_rows == 0)) &&
                    s.sm_steps <= 1 && !s.sm_symm && s.P.br == 1 && s.P.bc == 1 && h.coarse_n <= 512 && h.coarse_ld == h.coarse_n;
    if (!ok) break;
    --T;
  }
  return T > L - 2 ? -1 : T;              // (-1: no smoothed level qualifies)
}

// plain CSR copies of the tail levels' matrices (and the colour-major row lists of their Gauss-Seidel sweeps)
static void upload_tail_level(const amgx_level_desc& s, DevLevel& V) {
  const int64_t nnz = s.A.rowptr[s.A.n_rows];
  V.tA.upload(s.A); V.tP.upload(s.P); V.tPT.upload(s.PT);
  if (s.sm_type == AMGX_SM_JACOBI) {
    std::vector<double> sv((size_t)nnz);
    for (int64_t k = 0; k < nnz; ++k) sv[k] = s.A.val[k] * (s.omega * s.dinv[s.A.col[k]]);
    V.tApre.upload(s.A, sv.data());
  } else {
    std::vector<int32_t> cptr(s.n_colors + 1, 0), rl;
    for (int64_t i = 0; i < s.A.n_rows; ++i) if (s.color[i] >= 0) cptr[s.color[i] + 1]++;
    for (int c = 0; c < s.n_colors; ++c) cptr[c + 1] += cptr[c];
    rl.resize(cptr[s.n_colors]);
    std::vector<int32_t> pos(cptr.begin(), cptr.end() - 1);
    for (int64_t i = 0; i < s.A.n_rows; ++i) if (s.color[i] >= 0) rl[pos[s.color[i]]++] = (int32_t)i;
    V.t_rowlist.upload(rl); V.t_cptr.upload(cptr);
    V.t_rowcolor.upload(s.color, (size_t)s.A.n_rows);
  }
}

// ---- single-workgroup coarse tail: the program of tail_kernel for the levels >= T ----------
static void build_tail_program(Handle& h, const amgx_hierarchy_desc* d, const amgx_level_desc* levels) {
  const int L = d->n_levels;
  const int T = tail_first_level(h, d, levels);
  if (T <= 0) return;
  std::vector<TailOp> prog;
  const EpArgs none{nullptr, nullptr, nullptr, 0.0, nullptr, 0};
  auto spmv = [&](int ep, const DevCsr& M, int n, const double* x, double* y, EpArgs a) {
    prog.push_back(TailOp{T_SPMV, ep, n, M.rowptr.p, M.col.p, M.val.p, x, y, a, nullptr, nullptr, 0, 0, 0, nullptr});
  };
  auto gs = [&](DevLevel& V, int nc, int backward, int lds_ok) {
    prog.push_back(TailOp{T_GS, 0, (int)V.n, V.tA.rowptr.p, V.tA.col.p, V.tA.val.p, nullptr, V.x.p,
                          EpArgs{V.rhs.p, nullptr, V.dinv.p, 0.0, nullptr, 0}, V.t_rowlist.p, V.t_cptr.p, nc, backward, lds_ok, V.t_rowcolor.p});
  };
  auto gs_lds_ok = [&](int l) {
    const amgx_matrix& A = levels[l].A;
    if (A.n_rows > TAIL_BLOCK / TAIL_G || h.knobs.no_tail_lds) return 0;
    for (int64_t i = 0; i < A.n_rows; ++i) if (A.rowptr[i + 1] - A.rowptr[i] > TAIL_G * TAIL_GS_K) return 0;
    return 1;
  };
  for (int l = T; l + 1 < L; ++l) upload_tail_level(levels[l], h.lev[l]);
  h.tail_gs_lds.assign((size_t)L, -1);
  for (int l = T; l + 1 < L; ++l) if (h.lev[l].sm_type != AMGX_SM_JACOBI) h.tail_gs_lds[l] = gs_lds_ok(l);
  for (int l = T; l + 1 < L; ++l) {       // down
    DevLevel& V = h.lev[l];
    if (V.sm_type == AMGX_SM_JACOBI) {     // r = b - A'b, x = omega*Dinv*b
      spmv(EP_PRE, V.tApre, (int)V.n, V.rhs.p, V.res.p, EpArgs{V.rhs.p, nullptr, V.dinv.p, V.omega, V.x.p, 0});
    } else {                               // x = 0; forward sweep; r = b - A x
      prog.push_back(TailOp{T_ZERO, 0, (int)V.n, nullptr, nullptr, nullptr, nullptr, V.x.p, none, nullptr, nullptr, 0, 0, 0, nullptr});
      gs(V, levels[l].n_colors, 0, gs_lds_ok(l));
      spmv(EP_RES, V.tA, (int)V.n, V.x.p, V.res.p, EpArgs{V.rhs.p, nullptr, nullptr, 0.0, nullptr, 0});
    }
    spmv(EP_MULT, V.tPT, (int)h.lev[l + 1].n, V.res.p, h.lev[l + 1].rhs.p, none);   // b_{l+1} = P^T r
  }
  prog.push_back(TailOp{T_DENSE, 0, (int)h.coarse_n, nullptr, nullptr, h.coarse_inv.p, h.lev[L - 1].rhs.p, h.lev[L - 1].x.p,
                        none, nullptr, nullptr, 0, 0, 0, nullptr});
  for (int l = L - 2; l >= T; --l) {      // up
    DevLevel& V = h.lev[l];
    if (V.sm_type == AMGX_SM_JACOBI) {     // tmp = x + P x_{l+1} ; x = tmp + omega*Dinv*(b - A tmp)
      spmv(EP_AXPY, V.tP, (int)V.n, h.lev[l + 1].x.p, V.tmp.p, EpArgs{nullptr, V.x.p, nullptr, 1.0, nullptr, 0});
      spmv(EP_JAC, V.tA, (int)V.n, V.tmp.p, V.x.p, EpArgs{V.rhs.p, V.tmp.p, V.dinv.p, V.omega, nullptr, 0});
    } else {                               // x += P x_{l+1} ; backward sweep
      spmv(EP_AXPY, V.tP, (int)V.n, h.lev[l + 1].x.p, V.x.p, EpArgs{nullptr, V.x.p, nullptr, 1.0, nullptr, 0});
      gs(V, levels[l].n_colors, 1, gs_lds_ok(l));
    }
  }
  h.tail_prog.upload(prog);
  h.tail_ops = (int)prog.size();
  h.tail_level = T;
}

// ---- collapsed coarse levels (see dense_op_gemv_kernel) -----------------------------------------------------------
// Picks the first level l_c >= 1 from which the sub-cycle is cheaper as one dense GEMV than as its dependent launches,
// forms B column by column with the handle's own kernels (so B is exactly the operator the separate launches apply,
// whatever the smoother form) and stores it row-major.  AMGX_NO_DENSE_TAIL=1 disables, AMGX_DENSE_MAX=<n> caps n.
// first_level: 1 for a handle whose level 0 carries the caller's vectors; 0 for the replicated tail of a rank-partitioned
// hierarchy, where the whole handle may become one GEMV on the gathered vector
static void build_dense_tail(Handle& h, const amgx_hierarchy_desc* d, const amgx_level_desc* levels, int first_level = 1) {
  const int L = d->n_levels;
  if (d->cycle != AMGX_CYCLE_V || L < 2 + first_level || h.knobs.no_dense_tail) return;
  const int64_t cap = h.knobs.dense_max;
  for (int l = 0; l < L; ++l) if (h.lev[l].ncols != h.lev[l].n) return;       // rank-partitioned levels are driven stage by stage
  // dependent launches one cycle spends on level m (both directions), ~5 us each
  auto launches = [&](int m) -> double {
    const DevLevel& V = h.lev[m];
    const int k = std::max(1, V.sm_steps) * (V.sm_symm ? 2 : 1);
    if (V.sm_type == AMGX_SM_JACOBI) return V.paths.folded ? 3.0 : 2.0 + 3.0 * k;
    if (V.sm_type == AMGX_SM_CHEBY) return 3.0 + 2.0 * k * (V.cheb_degree + 1);
    if (V.sm_type == AMGX_SM_BGS) return 3.0 + 2.0 * k * std::max(1, V.bgs.n_colors);
    if (V.paths.hybrid()) return 2.0 + 3.0 * k;
    return 3.0 + 2.0 * k * std::max(1, V.gs.n_colors);
  };
  int lc = -1;
  double est = 5.0;                               // the coarse solve
  std::vector<double> est_from(L, 0.0);
  for (int m = L - 2; m >= first_level; --m) { est += 5.0 * launches(m); est_from[m] = est; }
  for (int m = first_level; m <= L - 2; ++m) {
    const int64_t N = h.lev[m].len();
    if (N < 1 || N > cap) continue;
    const double dense_us = 4.0 + 8.0 * (double)N * (double)N / 4.0e6;      // ~4 TB/s on a few hundred workgroups
    if (dense_us < 0.8 * est_from[m]) { lc = m; break; }
  }
  if (lc < first_level) return;
  const int N = (int)h.lev[lc].len();
  const int ld = (N + 1) & ~1;
  DevBuf<double> Bt;
  Bt.alloc((size_t)N * ld);
  h.dense_op.alloc((size_t)N * ld);
  HIPCHK(hipMemsetAsync(Bt.p, 0, (size_t)N * ld * sizeof(double), h.stream));
  HIPCHK(hipMemsetAsync(h.dense_op.p, 0, (size_t)N * ld * sizeof(double), h.stream));
  const int saved_tail = h.tail_level;
  h.tail_level = -1;                              // the sub-cycle runs as separate launches from level lc
  DevLevel& V = h.lev[lc];
  try {
    for (int j = 0; j < N; ++j) {
      launch(dense_unit_kernel, Handle::grid_for(N), BLOCK, 0, h.stream, (int64_t)N, (int64_t)j, V.rhs.p);
      h.cycle_v(V.x.p, V.rhs.p, lc);                // (dense_level is still -1: separate launches)
      HIPCHK(hipMemcpyAsync(Bt.p + (size_t)j * ld, V.x.p, (size_t)N * sizeof(double), hipMemcpyDeviceToDevice, h.stream));
      if ((j & 255) == 255) HIPCHK(hipStreamSynchronize(h.stream));          // bound the depth of the launch queue
    }
    const int tb = (N + 15) / 16;
    launch(dense_transpose_kernel, dim3(tb, tb), BLOCK, 0, h.stream, N, ld, Bt.p, h.dense_op.p);
    // leave the work vectors of the collapsed levels as create() made them
    for (int m = lc; m < L; ++m) {
      const size_t len = (size_t)std::max<int64_t>(1, h.lev[m].ext_len());
      for (double* v : {h.lev[m].x.p, h.lev[m].rhs.p, h.lev[m].res.p, h.lev[m].tmp.p}) HIPCHK(hipMemsetAsync(v, 0, len * sizeof(double), h.stream));
    }
    HIPCHK(hipStreamSynchronize(h.stream));
  } catch (...) { h.tail_level = saved_tail; throw; }
  h.tail_level = saved_tail;
  h.dense_level = lc;
  h.dense_n = N;
  h.dense_ld = ld;
}

// Chebyshev levels without an interval from the caller: lmax = 1.1 x a 30-step power-iteration estimate (defined next to the
// deterministic reductions it uses, at the end of amgx.hip)
static void cheb_estimate(Handle& h);

// K: the switches as the C-ABI entry point read them (Knobs::from_env, on the calling thread)
// dense_first: first level that may be collapsed into the dense operator (see build_dense_tail); < 0: never
static Handle* create(const amgx_hierarchy_desc* d, const Knobs& K, int dense_first = 1) {
  if (!d || d->n_levels < 1 || !d->levels) throw Err("amgx_create: empty hierarchy descriptor");
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev == 0) throw Err("amgx_create: no HIP device available (the apply path has no CPU fallback)");
  if (d->device < 0 || d->device >= ndev) throw Err("amgx_create: device ordinal out of range");
  HIPCHK(hipSetDevice(d->device));
  auto h = std::make_unique<Handle>();
  h->knobs = K;
  h->device = d->device;
  h->cycle = d->cycle;
  h->clev = d->clev;
  h->use_graph = d->use_graph != 0;
  h->ep_nt = (K.no_ep_nt ? 0 : EPF_NT) | (K.no_ep_hoist ? 0 : EPF_HOIST);   // A/B: -0.4 % cycle time (profiles/r01/restrict_fused.txt)
  if (d->cycle < 0 || d->cycle > 2) throw Err("amgx_create: unknown cycle");
  HIPCHK(hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking));
  h->stream = h->own_stream;
  h->lev.resize(d->n_levels);
  std::vector<amgx_level_desc> pl(d->levels, d->levels + d->n_levels);
  std::vector<LevelPerm> pstore(d->n_levels);
  permute_gs_levels(K, d, pl, pstore);
  SetupClock clk(K);
  clk.lap("renumbering of Gauss-Seidel levels");
  h->perm.resize(d->n_levels);
  for (int l = 0; l < d->n_levels; ++l) if (!pstore[l].perm.empty()) h->perm[l].upload(pstore[l].perm);
  const amgx_level_desc* levels = pl.data();
  for (int l = 0; l < d->n_levels; ++l) {
    LevelBuild B{h->knobs, clk, levels[l], l + 1 < d->n_levels ? &levels[l + 1] : nullptr, h->lev[l], l, d->cycle, dense_first, d->n_levels};
    check_level(B);
    SetupTasks tasks(d->device, K);       // (after B: see LevelBuild)
    upload_level_matrix(B, tasks);
    if (!B.last()) {
      upload_transfers(B, tasks);
      build_smoother_data(B, tasks);
      if (B.s.sm_type == AMGX_SM_JACOBI && B.s.A.br == 1 && B.s.sm_steps <= 1 && !B.s.sm_symm) build_jacobi_down(B, tasks);
      build_folded_prolongation(B, tasks);
      tasks.wait();
      cheb_fused_restrict(B);
      clk.lap("level images (A, P, P^T, smoother data, A', Q: concurrent host tasks)", l);
    } else if (B.s.dinv) {
      tasks.wait();
      build_coarsest_smoother_data(B);
    }
    tasks.wait();
    mat_f32_image(B);
    set_xcd_modes(B);
    alloc_level_vectors(B);
    resolve_paths(B.L);                   // every image of the level is final here; nothing before this line runs a cycle or asks folded()
    allow_down_nv_lw(B.L);
  }
  // (the levels of a rank-partitioned hierarchy are estimated collectively, on the partitioned operator: amgx_dist_cheb_estimate)
  if (dense_first >= 0) cheb_estimate(*h);
  clk.lap("Chebyshev intervals (power iteration)");
  if (d->clev == AMGX_CLEV_INV) build_coarse_inverse(*h, d, levels[d->n_levels - 1]);
  build_tail_program(*h, d, levels);
  HIPCHK(hipDeviceSynchronize());
  clk.lap("coarse inverse, tail program");
  if (dense_first >= 0) build_dense_tail(*h, d, levels, dense_first);
  clk.lap("collapsed coarse levels (dense operator)");
  return h.release();
}

}  // namespace amgx
