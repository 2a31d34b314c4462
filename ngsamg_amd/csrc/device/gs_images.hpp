// Builders of the Gauss-Seidel images (included by amgx.hip after devbuild.hpp): build_gs (multicolour), build_gsb (block-hybrid,
// scalar levels), build_bgsb (block-hybrid, square-block levels) and their AMGX_VERIFY_IMAGES cross-checks.  The structs they fill
// (DevGS, DevGSB, DevBGSB) stay with Handle, where they are read.
//
// Which entries an image keeps is stated once, in devbuild.hpp, for the host loops here and the device kernels there:
// db_split_part (the two parts of the scalar split) and db_bsell_keep / db_bsell_col / db_bsell_factor (the BB_* images of a block
// level).  A builder here decides the row list and the `sel` value of an image and where it is formed -- on the device from the
// CSR arrays that are already there (big levels), else by the host loops.  DESIGN.md 6: how to add a Gauss-Seidel image.
#pragma once

namespace amgx {

// ---- shared steps -----------------------------------------------------------------------------------

// Rows of equal colour inside one unit of the sweep must not be coupled (the parallel sweep would race).  same_unit(i, j): rows i
// and j are swept by one unit (always / the same run of B rows / the same sweep block); ghost columns (j >= n) are frozen during
// the sweep and never count.  `coupled`: the message of the builder that asks.
template <class SameUnit>
static void check_colouring(const amgx_matrix& A, const int32_t* color, int nc, SameUnit same_unit, const char* coupled) {
  const int64_t n = A.n_rows;
  std::vector<char> bad(setup_threads(), 0);
  par_for(n, [&](int64_t i0, int64_t i1, int t) {
    for (int64_t i = i0; i < i1; ++i) {
      const int ci = color[i];
      if (ci >= nc) { bad[t] = 1; return; }
      if (ci < 0) continue;
      for (int64_t k = A.rowptr[i]; k < A.rowptr[i + 1]; ++k) {
        const int64_t j = A.col[k];
        if (j != i && j < n && color[j] == ci && same_unit(i, j)) { bad[t] = 2; return; }
      }
    }
  });
  for (char c : bad) if (c == 1) throw Err("colour index out of range");
  for (char c : bad) if (c == 2) throw Err(coupled);
}

// widest slice of a SELL image (steps of 64 lanes) from its slice pointers
static int sell_max_width(const std::vector<int64_t>& slice_ptr) {
  int mw = 0;
  for (size_t q = 0; q + 1 < slice_ptr.size(); ++q)
    mw = std::max(mw, (int)(((slice_ptr[q + 1] & ~(int64_t)63) - (slice_ptr[q] & ~(int64_t)63)) / WAVE));
  return mw;
}

// colour-major list of the coloured rows, every colour padded with -1 to a multiple of R slots: colour c is start[c] .. start[c + 1]
struct ColourRows {
  std::vector<int32_t> rows;
  std::vector<int64_t> start;
};
static ColourRows colour_major_rows(const int32_t* color, int64_t n, int nc, int R) {
  ColourRows o;
  o.start.assign(nc + 1, 0);
  for (int64_t i = 0; i < n; ++i) if (color[i] >= 0) o.start[color[i] + 1]++;
  for (int c = 0; c < nc; ++c) o.start[c + 1] = o.start[c] + ((o.start[c + 1] + R - 1) / R) * R;
  o.rows.assign(o.start[nc], -1);
  std::vector<int64_t> pos(o.start.begin(), o.start.end() - 1);
  for (int64_t i = 0; i < n; ++i) if (color[i] >= 0) o.rows[pos[color[i]]++] = (int32_t)i;
  return o;
}

// lower (part 0) / upper (part 1) part of A w.r.t. the colour order, blocks of bb values; couplings to non-free columns are
// dropped (x is 0 there), non-free rows are empty
static HostCsr colour_part(const amgx_matrix& A, const int32_t* color, int part, int bb) {
  const int64_t n = A.n_rows, nnz = A.rowptr[n];
  HostCsr F;
  F.rowptr.assign(n + 1, 0);
  F.col.reserve(nnz / 2 + 16); F.val.reserve((nnz / 2 + 16) * bb);
  for (int64_t i = 0; i < n; ++i) {
    const int ci = color[i];
    if (ci >= 0)
      for (int64_t k = A.rowptr[i]; k < A.rowptr[i + 1]; ++k) {
        const int cj = color[A.col[k]];
        if (cj < 0) continue;
        if ((part == 0 && cj < ci) || (part == 1 && cj > ci)) {
          F.col.push_back(A.col[k]);
          F.val.insert(F.val.end(), A.val + k * bb, A.val + (k + 1) * bb);
        }
      }
    F.rowptr[i + 1] = (int64_t)F.col.size();
  }
  return F;
}
static amgx_matrix with_csr(amgx_matrix M, const HostCsr& c) { use_csr(M, c); return M; }

// ---- multicolour Gauss-Seidel -----------------------------------------------------------------------

// dinv is the plain inverse of the diagonal (block) on every coloured row: the split forms rely on x_k = (b - L x)_k / a_kk
static bool gs_plain_diag(const amgx_level_desc& d) {
  const int64_t n = d.A.n_rows;
  const int bs = d.A.br, bb = bs * bs;
  for (int64_t i = 0; i < n; ++i) {
    if (d.color[i] < 0) continue;
    const double* aii = nullptr;
    for (int64_t k = d.A.rowptr[i]; k < d.A.rowptr[i + 1]; ++k) if (d.A.col[k] == i) aii = d.A.val + k * bb;
    const double* di = d.dinv + i * bb;
    if (bs == 1) { if (!(std::fabs(di[0] * (aii ? aii[0] : 0.0) - 1.0) < 1e-12)) return false; continue; }
    if (!aii) return false;
    for (int r = 0; r < bs; ++r)
      for (int c = 0; c < bs; ++c) {
        double v = 0.0;
        for (int q = 0; q < bs; ++q) v += di[r * bs + q] * aii[q * bs + c];
        if (!(std::fabs(v - (r == c ? 1.0 : 0.0)) < 1e-10)) return false;
      }
  }
  return true;
}

static void build_gs(const Knobs& K, const amgx_level_desc& d, DevLevel& L) {
  const int64_t n = d.A.n_rows;
  if (!d.color || d.n_colors <= 0) { if (n > 0) throw Err("AMGX_SM_GS needs a row colouring (color / n_colors)"); return; }
  const int nc = d.n_colors;
  check_colouring(d.A, d.color, nc, [](int64_t, int64_t) { return true; }, "invalid colouring: two coupled rows share a colour");
  DevGS& g = L.gs;
  g.n_colors = nc;
  const bool square_dinv = d.dinv != nullptr && d.A.n_rows == d.A.n_cols;
  if (d.A.br == 1) {
    // lanes per row: one thread per row only while a colour still has >= 2^17 rows; below that G grows with the row
    // length so that a row is consumed in ~2-4 steps
    const double avg = n ? (double)d.A.rowptr[n] / (double)n : 0.0;
    int G = 1;
    if (n / std::max(1, nc) < ((int64_t)1 << 17)) while (G < 16 && avg > 4.0 * G) G <<= 1;
    g.lanes = G;
    const int R = WAVE / G;
    // colour-major row list, each colour padded to a multiple of R rows (= whole slices)
    const ColourRows cr = colour_major_rows(d.color, n, nc, R);
    g.color_slice_ptr.resize(nc + 1);
    for (int c = 0; c <= nc; ++c) g.color_slice_ptr[c] = (int)(cr.start[c] / R);
    HostSell S;
    // (absolute 16-bit column bases, not row-relative: the row product then does not depend on the rowid load)
    build_sell(d.A, cr.rows.data(), (int64_t)cr.rows.size(), K.gs_rowrel, G, S);
    upload_sell(S, g.sell);
    g.rowid.upload(cr.rows);
    g.n_slices_total = (int)(S.slice_ptr.size() - 1);
    if (!(square_dinv && gs_plain_diag(d))) return;
    for (int part = 0; part < 2; ++part) {
      const HostCsr F = colour_part(d.A, d.color, part, 1);
      HostSell SP;
      build_sell(with_csr(d.A, F), cr.rows.data(), (int64_t)cr.rows.size(), K.gs_rowrel, G, SP);
      if ((int)(SP.slice_ptr.size() - 1) != g.n_slices_total) throw Err("build_gs: split copy has a different slice count");
      upload_sell(SP, part == 0 ? g.lower : g.upper);
    }
    g.has_split = true;
    return;
  }
  const ColourRows list = colour_major_rows(d.color, n, nc, 1);
  g.color_row_ptr.assign(list.start.begin(), list.start.end());
  g.rowlist.upload(list.rows);
  // colour-major BSELL copy: every colour padded to whole slices of RB block rows (big levels: one more copy of A,
  // 2x the sweep speed; small levels keep the CSR row-list kernel: their colours are shorter than a slice)
  const int bs = d.A.br;
  if (!((bs == 2 || bs == 3 || bs == 6) && n / std::max(1, nc) >= K.bgs_bsell_min && !K.no_bgs_bsell)) return;
  const int RB = WAVE / bs;
  const ColourRows cr = colour_major_rows(d.color, n, nc, RB);
  if (!build_bsell(d.A, g.bcopy, 1.6, cr.rows.data(), (int64_t)cr.rows.size())) return;
  g.color_slice_ptr.resize(nc + 1);
  for (int c = 0; c <= nc; ++c) g.color_slice_ptr[c] = (int)(cr.start[c] / RB);
  g.rowid.upload(cr.rows);
  g.bsell_ok = true;
  // split copies (see the scalar case): need x_B = Dinv_B (b - L x)_B to imply (b - L x - D x)_B = 0, i.e. Dinv_B = A_BB^-1
  if (!(square_dinv && !K.no_bgs_split && gs_plain_diag(d))) return;
  bool ok = true;
  for (int part = 0; part < 2 && ok; ++part) {
    const HostCsr F = colour_part(d.A, d.color, part, bs * bs);
    DevMatrix& T = part == 0 ? g.blower : g.bupper;
    ok = build_bsell(with_csr(d.A, F), T, 1e9, cr.rows.data(), (int64_t)cr.rows.size()) && T.n_slices == g.bcopy.n_slices;
  }
  g.bsplit = ok;
}

// ---- block-hybrid Gauss-Seidel, scalar levels (gsb_sweep_kernel) ------------------------------------

// local-window image of the colour-sorted block image `full` (gsb_sweep_kernel<..., LW>): per block of B rows the sorted list of its
// distinct off-block columns; entries carry codes (in-block: row - r0 < B; off-block: B + position in the list).  Blocks whose list
// exceeds GSB_LW_CAP keep global 32-bit columns.  rows: the slot -> row list of the block image (-1 = padding), slots = n_blocks * B.
static bool build_gsb_full_lw(const Knobs& K, const amgx_matrix& A, const std::vector<int32_t>& rows, int64_t slots, int B, int G, DevGSB& g) {
  const int64_t n = A.n_rows, nnz = A.rowptr[n];
  const int64_t nb = (n + B - 1) / B;
  std::vector<int32_t> cnt((size_t)nb + 1, 0);
  RawVec<int32_t> code;
  code.resize((size_t)std::max<int64_t>(1, nnz));
  std::vector<std::vector<int32_t>> lists((size_t)nb);
  std::vector<char> no16((size_t)n, 0);
  std::vector<int64_t> n_over(setup_threads(), 0);
  const int64_t cap = K.lw_cap_small(GSB_LW_CAP);
  const bool tcap = K.lw_test_cap_on;
  par_for(nb, [&](int64_t b0, int64_t b1, int t) {
    std::vector<int32_t> u;
    for (int64_t kb = b0; kb < b1; ++kb) {
      const int64_t r0 = kb * B, r1 = std::min<int64_t>(n, r0 + B);
      u.clear();
      for (int64_t k = A.rowptr[r0]; k < A.rowptr[r1]; ++k) if (A.col[k] < r0 || A.col[k] >= r1) u.push_back(A.col[k]);
      std::sort(u.begin(), u.end());
      u.erase(std::unique(u.begin(), u.end()), u.end());
      if ((int64_t)u.size() > cap) {
        for (int64_t i = r0; i < r1; ++i) no16[i] = 1;
        for (int64_t k = A.rowptr[r0]; k < A.rowptr[r1]; ++k) code[k] = A.col[k];
        n_over[t]++;
        continue;
      }
      for (int64_t k = A.rowptr[r0]; k < A.rowptr[r1]; ++k) {
        const int32_t j = A.col[k];
        code[k] = (j >= r0 && j < r1) ? (int32_t)(j - r0) : (int32_t)(B + (std::lower_bound(u.begin(), u.end(), j) - u.begin()));
      }
      cnt[kb + 1] = (int32_t)u.size();
      lists[kb] = u;
    }
  }, 16);
  int64_t overs = 0;
  for (int64_t v : n_over) overs += v;
  if (overs * 20 > nb && !tcap) return false;
  for (int64_t kb = 0; kb < nb; ++kb) cnt[kb + 1] += cnt[kb];
  std::vector<int32_t> ccol((size_t)std::max<int32_t>(1, cnt[nb]));
  par_for(nb, [&](int64_t b0, int64_t b1, int) { for (int64_t kb = b0; kb < b1; ++kb) std::copy(lists[kb].begin(), lists[kb].end(), ccol.begin() + cnt[kb]); }, 64);
  amgx_matrix Lm = A;
  Lm.col = code.data();
  HostSell S;
  build_sell(Lm, rows.data(), slots, false, G, S, false, &no16);
  // every slice must fit the kernel's register budget exactly like `full` (same widths: same rows, same lengths)
  upload_sell(S, g.fullLW);
  g.flw_cptr.upload(cnt);
  g.flw_ccol.upload(ccol);
  g.has_fullLW = true;
  g.flw_no_window = overs;
  return true;
}

// The split of A for the pre-smoothing from zero (db_split_part): part 0 = in-block couplings to lower colours, part 1 = everything
// else but the diagonal; couplings to non-free columns are dropped (x is 0 there), non-free rows are empty (their residual is not
// needed: their prolongation rows are empty).  The host and the device source of build_gsb_images differ in these calls only:
enum : int { GSB_WHOLE = -1 };
struct GsbSource {
  // SELL image over the block image's slot list of part q (GSB_WHOLE: of A itself) into `out`; returns its slice pointers
  std::function<std::vector<int64_t>(int q, DevMatrix::Sell& out)> image;
  // forms the two parts and cvec; false: a swept row has no diagonal inverse (no split)
  std::function<bool(DevBuf<double>& cvec)> split;
  std::function<const amgx_matrix&()> host1;     // part 1 as host arrays (the device source downloads them once)
  const DevCsrSrc* dev1 = nullptr;               // part 1 on the device, where it was formed there
};

struct GsbHostParts {
  std::vector<int64_t> rp[2];
  RawVec<int32_t> cc[2];
  RawVec<double> vv[2];
  amgx_matrix F[2];
};
static GsbSource gsb_host_source(const amgx_level_desc& d, int B, int G, const std::vector<int32_t>& rows, GsbHostParts& S) {
  const int64_t n = d.A.n_rows;
  GsbSource src;
  src.image = [&d, &rows, &S, G](int q, DevMatrix::Sell& out) {
    HostSell H;
    build_sell(q == GSB_WHOLE ? d.A : S.F[q], rows.data(), (int64_t)rows.size(), false, G, H);
    upload_sell(H, out);
    return std::move(H.slice_ptr);
  };
  src.split = [&d, &S, n, B](DevBuf<double>& cvec) {
    const DbSplit a{n, B, d.A.rowptr, d.A.col, d.A.val, d.color, d.dinv};
    std::vector<double> cv((size_t)n, 0.0);
    for (int part = 0; part < 2; ++part) S.rp[part].assign(n + 1, 0);
    par_for(n, [&](int64_t i0, int64_t i1, int) {
      for (int64_t i = i0; i < i1; ++i) {
        const int ci = d.color[i];
        if (ci < 0) continue;
        for (int64_t k = d.A.rowptr[i]; k < d.A.rowptr[i + 1]; ++k) {
          const int pt = db_split_part(a, i, ci, d.A.col[k]);
          if (pt >= 0) S.rp[pt][i + 1]++;
        }
      }
    });
    for (int part = 0; part < 2; ++part) {
      for (int64_t i = 0; i < n; ++i) S.rp[part][i + 1] += S.rp[part][i];
      S.cc[part].resize((size_t)std::max<int64_t>(1, S.rp[part][n]));
      S.vv[part].resize((size_t)std::max<int64_t>(1, S.rp[part][n]));
    }
    std::vector<char> bad(setup_threads(), 0);
    par_for(n, [&](int64_t i0, int64_t i1, int t) {
      for (int64_t i = i0; i < i1; ++i) {
        const int ci = d.color[i];
        if (ci < 0) continue;
        int64_t o[2] = {S.rp[0][i], S.rp[1][i]};
        double aii = 0.0;
        for (int64_t k = d.A.rowptr[i]; k < d.A.rowptr[i + 1]; ++k) {
          const int64_t j = d.A.col[k];
          if (j == i) { aii = d.A.val[k]; continue; }
          const int pt = db_split_part(a, i, ci, j);
          if (pt < 0) continue;
          S.cc[pt][o[pt]] = (int32_t)j; S.vv[pt][o[pt]] = d.A.val[k]; ++o[pt];
        }
        if (d.dinv[i] != 0.0) cv[i] = 1.0 / d.dinv[i] - aii; else bad[t] = 1;     // a swept row without a diagonal inverse
      }
    });
    for (char c : bad) if (c) return false;
    for (int part = 0; part < 2; ++part) { S.F[part] = d.A; S.F[part].rowptr = S.rp[part].data(); S.F[part].col = S.cc[part].data(); S.F[part].val = S.vv[part].data(); }
    cvec.upload(cv);
    return true;
  };
  src.host1 = [&S]() -> const amgx_matrix& { return S.F[1]; };
  return src;
}

struct GsbDevParts {
  DevCsrSrc part[2];
  HostCsr h1;                                    // part 1 on the host, once somebody asks
  amgx_matrix F1;
};
// csr: the level matrix on the device; d_rows: the slot list there; d_dinv: dinv there
static GsbSource gsb_dev_source(const amgx_level_desc& d, int B, int G, const DevCsrSrc& csr, const int32_t* d_rows, int64_t slots, const double* d_dinv,
                                GsbDevParts& S) {
  const int64_t n = d.A.n_rows;
  GsbSource src;
  src.image = [&csr, &S, d_rows, slots, G](int q, DevMatrix::Sell& out) {
    const DevCsrSrc& M = q == GSB_WHOLE ? csr : S.part[q];
    DevBuf<int64_t> sp;
    const int64_t stored = dev_slice_offsets(M, d_rows, slots, sp, G);
    dev_build_sell(M, d_rows, slots, G, false, false, nullptr, 0.0, nullptr, sp, stored, out, nullptr);
    return db_download(out.slice_ptr, out.slice_ptr.n);
  };
  src.split = [&d, &csr, &S, n, B, d_dinv](DevBuf<double>& cvec) {
    DevBuf<int32_t> dcolor;
    dcolor.upload(d.color, (size_t)n);
    const DbSplit a{n, B, csr.rowptr.p, csr.col.p, csr.val.p, dcolor.p, d_dinv};
    DevCsrSrc* part = S.part;
    for (int q = 0; q < 2; ++q) { part[q].n_rows = n; part[q].n_cols = d.A.n_cols; part[q].rowptr.alloc((size_t)n + 1); }
    const unsigned grid = (unsigned)((n + BLOCK - 1) / BLOCK);
    launch(db_split_count_kernel, grid, BLOCK, 0, 0, a, part[0].rowptr.p, part[1].rowptr.p);
    for (int q = 0; q < 2; ++q) {
      launch(db_scan_kernel, 1, 1024, 0, 0, n, part[q].rowptr.p);
      HIPCHK(hipMemcpy(&part[q].nnz, part[q].rowptr.p + n, sizeof(int64_t), hipMemcpyDeviceToHost));
      part[q].col.alloc((size_t)std::max<int64_t>(1, part[q].nnz));
      part[q].val.alloc((size_t)std::max<int64_t>(1, part[q].nnz));
    }
    cvec.alloc((size_t)n);
    DevBuf<int> bad;
    bad.alloc(1);
    HIPCHK(hipMemset(bad.p, 0, sizeof(int)));
    launch(db_split_fill_kernel, grid, BLOCK, 0, 0, a, part[0].rowptr.p, part[1].rowptr.p, part[0].col.p, part[0].val.p,
                       part[1].col.p, part[1].val.p, cvec.p, bad.p);
    int hbad = 0;
    HIPCHK(hipMemcpy(&hbad, bad.p, sizeof(int), hipMemcpyDeviceToHost));
    return hbad == 0;
  };
  src.host1 = [&d, &S, n]() -> const amgx_matrix& {
    if (S.h1.rowptr.empty()) {
      const size_t nnz1 = (size_t)std::max<int64_t>(1, S.part[1].nnz);
      S.h1.rowptr = db_download(S.part[1].rowptr, (size_t)n + 1);
      S.h1.col = db_download(S.part[1].col, nnz1);
      S.h1.val = db_download(S.part[1].val, nnz1);
      S.F1 = with_csr(d.A, S.h1);
    }
    return S.F1;
  };
  src.dev1 = &S.part[1];
  return src;
}

// Block-hybrid Gauss-Seidel data (gsb_sweep_kernel).  Validated like the colourings above: two coupled rows of one block
// sharing a colour would be a data race.
// csr: the level matrix on the device (big levels): the images and the split are then formed there (devbuild.hpp)
static void build_gsb_images(const Knobs& K, const amgx_level_desc& d, DevLevel& L, const amgx_matrix* P, const DevCsrSrc* csr) {
  const int64_t n = d.A.n_rows;
  DevGSB& g = L.gsb;
  const int B = d.gs_block_rows;
  // ---- shape: lanes per row from the longest row (a lane holds <= 16 entries, + 1 when G = 1); workgroup size TH = B * G
  int64_t mx = 0;
  {
    std::vector<int64_t> tmx(setup_threads(), 0);
    par_for(n, [&](int64_t i0, int64_t i1, int t) { int64_t m = 0; for (int64_t i = i0; i < i1; ++i) m = std::max<int64_t>(m, d.A.rowptr[i + 1] - d.A.rowptr[i]); tmx[t] = m; });
    for (int64_t v : tmx) mx = std::max(mx, v);
  }
  int G = 1;
  while (G < 16 && mx > 16 * G + (G == 1 ? 1 : 0)) G <<= 1;
  // the ranks of a partitioned level agree on ONE block size (the smallest any of them needs, dist.py) while their longest
  // rows may differ: a rank with shorter rows spreads them over more lanes than it must, so that B * G is a workgroup size
  while (G < 16 && B >= 16 && B * G < 256) G <<= 1;
  if (n == 0) {                     // a rank that owns nothing: the form is "on" (the cycle drivers test it) with no block to sweep
    g.B = B > 0 ? B : 256; g.G = 1; g.TH = 256; g.n_colors = 0; g.n_blocks = 0;
    return;
  }
  const int TH = B * G;
  if (B < 16 || (TH != 256 && TH != 512 && TH != 1024))
    throw Err("gs_block_rows = " + std::to_string(B) + " with " + std::to_string(G) + " lanes per row (longest row: " + std::to_string(mx) +
              " entries) does not give a workgroup of 256, 512 or 1024 lanes");
  if (d.A.br != 1 || d.A.bc != 1) throw Err("block-hybrid Gauss-Seidel: scalar levels only");
  if (!d.color || d.n_colors <= 0 || d.n_colors > 254) { if (n > 0) throw Err("block-hybrid Gauss-Seidel needs a blocked colouring with at most 254 colours"); return; }
  if (!d.dinv) throw Err("dinv missing");
  const int nc = d.n_colors;
  // ---- validate
  check_colouring(d.A, d.color, nc, [B](int64_t i, int64_t j) { return i / B == j / B; },
                  "invalid blocked colouring: two coupled rows of one block share a colour");
  g.B = B; g.G = G; g.TH = TH; g.n_colors = nc;
  g.n_blocks = (int)((n + B - 1) / B);
  // ---- slot order: the rows of every block sorted by colour (stable), rows that are never swept last
  const int64_t slots = (int64_t)g.n_blocks * B;
  std::vector<int32_t> rows((size_t)slots, -1);
  std::vector<uint8_t> sc((size_t)slots, 255);
  par_for(g.n_blocks, [&](int64_t k0, int64_t k1, int) {
    for (int64_t kb = k0; kb < k1; ++kb) {
      const int64_t b0 = kb * B, b1 = std::min<int64_t>(n, b0 + B);
      for (int64_t i = b0; i < b1; ++i) rows[i] = (int32_t)i;
      std::stable_sort(rows.begin() + b0, rows.begin() + b1, [&](int32_t a, int32_t c) {
        return (d.color[a] < 0 ? 255 : d.color[a]) < (d.color[c] < 0 ? 255 : d.color[c]); });
      for (int64_t q = b0; q < b1; ++q) sc[q] = d.color[rows[q]] < 0 ? 255 : (uint8_t)d.color[rows[q]];
    }
  }, 16);
  g.rowid.upload(rows);
  g.slotcolor.upload(sc);
  auto checked_width = [&](const std::vector<int64_t>& slice_ptr, const char* what) {
    const int mw = sell_max_width(slice_ptr);
    if (mw > 2 * GSB_WP + 1) throw Err(std::string("block-hybrid Gauss-Seidel (") + what + "): a row has more than " + std::to_string((2 * GSB_WP) * G + 1) +
                                       " entries for gs_block_rows = " + std::to_string(B) + " (use smaller blocks)");
    return mw;
  };
  const double avgA = (double)d.A.rowptr[n] / (double)n;
  const bool long_rows = avgA >= 24.0 && K.lw_wanted(n) && d.A.n_cols == n;
  // ---- full (+ fullLW: long-row square levels, local-window image of `full` for the general sweep)
  // Measured NON-win at cfg 2 (profiles/r04/gs_experiments.txt): level-1 backward sweep 231 us with the window against 196 us without
  // (the extra barrier and the window's registers cost more than the gathers of the off-block values, which this kernel issues
  // back to back in one burst).  Built and tested, off unless AMGX_GSB_LW=1.
  if (long_rows && G > 1 && K.gsb_lw) build_gsb_full_lw(K, d.A, rows, slots, B, G, g);
  GsbHostParts hparts;
  GsbDevParts dparts;
  GsbSource src;
  if (csr) src = gsb_dev_source(d, B, G, *csr, g.rowid.p, slots, L.dinv.p, dparts);
  else src = gsb_host_source(d, B, G, rows, hparts);
  g.full_maxw = checked_width(src.image(GSB_WHOLE, g.full), "A");
  // ---- split into two CSR parts (+ cvec)
  if (!src.split(g.cvec) || K.gsb_no_split) { g.cvec.release(); return; }
  // ---- the images of the sweep from zero: lowin, rest (device builder first; the CSR fallback for a badly padded remainder is the
  // host builder's)
  g.lowin_maxw = checked_width(src.image(0, g.lowin), "lower part");
  if (!(src.dev1 && dev_upload_matrix(K, *src.dev1, g.rest, false, 1.6, SELL_WIN, nullptr)))
    upload_matrix(K, src.host1(), g.rest, "A (block-hybrid Gauss-Seidel: rest)", true, false, false, 1.6, SELL_WIN);
  g.has_split = true;
  // ---- restLW (long-row levels: local-window image of the rest part) and the restriction RG that goes with it
  if (P && long_rows && K.fused_restrict_ok(*P, 1)) {
    // (device builder first, devbuild.hpp dev_build_lw; the host builder works from the host arrays of the part)
    auto host_lw = [&](int gg, DevMatrix& M, DevBuf<int32_t>& cp, DevBuf<int32_t>& cl) {
      const amgx_matrix& F = src.host1();
      return build_sell_lw(K, F, F.val, gg, M, cp, cl);
    };
    auto drop_lw = [&] { g.restLW = DevMatrix(); g.lw_cptr.release(); g.lw_ccol.release(); };
    const bool dev_lw = src.dev1 && !K.host_lw;
    int GL = 0;
    for (int gg : values(DownLwLanes{})) {
      bool ok = false;
      if (dev_lw) {
        ok = dev_build_lw(*src.dev1, false, gg, K.lw_cap(LW_CAP), K.lw_test_cap_on, nullptr, 0.0, g.restLW, g.lw_cptr, g.lw_ccol);
        if (ok && K.verify_images) {
          DevMatrix H; DevBuf<int32_t> hp, hc;
          if (!host_lw(gg, H, hp, hc)) throw Err("AMGX_VERIFY_IMAGES: Gauss-Seidel rest (local window): the host builder declines what the device builder forms");
          verify_same_lw(g.restLW, g.lw_cptr, g.lw_ccol, H, hp, hc, "Gauss-Seidel rest (local window)");
        }
        if (!ok) drop_lw();
      }
      if (!ok) ok = host_lw(gg, g.restLW, g.lw_cptr, g.lw_ccol);
      if (ok) { GL = gg; break; }
      g.restLW = DevMatrix();
    }
    if (GL) {
      build_restrict(K, *P, L.RG, 512 / GL, 4 * 512, 512);
      if (!L.RG.empty()) return;
      drop_lw();
    }
  }
  if (P && g.rest.fmt == FMT_SELL && g.rest.lanes == 1 && K.fused_restrict_ok(*P, 1))
    build_restrict(K, *P, L.RG, 512, 6 * 512);
}

static void build_gsb(const Knobs& K, const amgx_level_desc& d, DevLevel& L, const amgx_matrix* P, const DevCsrSrc* csr = nullptr) {
  build_gsb_images(K, d, L, P, csr);
  gsb_set_paths(K, L.gsb);
}

// ---- block-hybrid Gauss-Seidel, square-block levels (bgsb_sweep_kernel) -----------------------------

// BSELL image of selected entries of a square-block matrix: `rows` lists block rows in storage order (-1 = padding slot), slices of
// RB = 64 / bs consecutive list entries.  sel (BB_*, devbuild.hpp) with the maps of the sweep blocks says which entries the image
// keeps, the block column it stores for them and the factor on their values; padding steps carry column 0.  The host side of
// dev_build_bsell: same rule functions, same layout.
static void build_bsell_sel(const amgx_matrix& A, const std::vector<int32_t>& rows, int sel, const DbBgsbMaps& mp, DevMatrix& D) {
  const int bs = A.br;
  const int RB = WAVE / bs;
  const int64_t n = A.n_rows, m = (int64_t)rows.size();
  if (m % RB) throw Err("build_bsell_sel: the row list must be padded to whole slices");
  const int64_t ns = m / RB;
  std::vector<int64_t> sp(ns + 1, 0);
  par_for(ns, [&](int64_t s0, int64_t s1, int) {
    for (int64_t s = s0; s < s1; ++s) {
      int w = 0;
      for (int rb = 0; rb < RB; ++rb) {
        const int32_t i = rows[s * RB + rb];
        if (i < 0) continue;
        int c = 0;
        for (int64_t k = A.rowptr[i]; k < A.rowptr[i + 1]; ++k) if (db_bsell_keep(mp, n, sel, i, A.col[k])) ++c;
        w = std::max(w, c);
      }
      sp[s + 1] = w;
    }
  }, 16);
  for (int64_t s = 0; s < ns; ++s) sp[s + 1] += sp[s];
  const int64_t steps = sp[ns];
  RawVec<int32_t> col;
  RawVec<double> val;
  par_assign(col, (size_t)std::max<int64_t>(1, steps * RB), (int32_t)0);
  par_assign(val, (size_t)std::max<int64_t>(1, steps * bs * WAVE), 0.0);
  par_for(ns, [&](int64_t s0, int64_t s1, int) {
    for (int64_t s = s0; s < s1; ++s)
      for (int rb = 0; rb < RB; ++rb) {
        const int32_t i = rows[s * RB + rb];
        if (i < 0) continue;
        int64_t kk = sp[s];
        for (int64_t k = A.rowptr[i]; k < A.rowptr[i + 1]; ++k) {
          const int32_t j = A.col[k];
          if (!db_bsell_keep(mp, n, sel, i, j)) continue;
          col[kk * RB + rb] = db_bsell_col(mp, sel, j);
          const double* blk = A.val + k * bs * bs;
          const double sc = db_bsell_factor(mp, sel, i, j);
          double* vk = val.data() + kk * (bs * WAVE);
          for (int rr = 0; rr < bs; ++rr) {
            const int lane = rb * bs + rr;
            for (int c = 0; c < bs; ++c) {
              if ((bs & 1) && c == bs - 1) vk[(bs / 2) * (2 * WAVE) + lane] = sc * blk[rr * bs + c];
              else vk[(c / 2) * (2 * WAVE) + lane * 2 + (c & 1)] = sc * blk[rr * bs + c];
            }
          }
          ++kk;
        }
      }
  }, 16);
  D.fmt = FMT_BSELL; D.br = D.bc = bs;
  D.n_rows = A.n_rows; D.n_cols = A.n_cols;
  D.n_slices = (int)ns;
  D.stored = steps * RB;
  D.stream_bytes = steps * ((int64_t)bs * WAVE * 8 + RB * 4) + 8 * (ns + 1);
  D.bsell.slice_ptr.upload(sp); D.bsell.col.upload(col); D.bsell.val.upload(val);
}

// sweep blocks of a block level: runs of BB consecutive rows, or the caller's compact blocks (gs_block_ids, at most BB rows each)
struct SweepBlocks {
  int n = 0;
  std::vector<int32_t> of, lpos, ptr, rows;      // block of every row, its position there; rows[ptr[q] .. ptr[q + 1]): the rows of block q
};
static SweepBlocks bgsb_sweep_blocks(const amgx_level_desc& d) {
  const int64_t n = d.A.n_rows;
  const int BB = d.gs_block_rows;
  SweepBlocks b;
  b.of.resize((size_t)n); b.lpos.resize((size_t)n); b.rows.resize((size_t)n);
  if (d.gs_block_ids) {
    int32_t mx = -1;
    for (int64_t i = 0; i < n; ++i) { if (d.gs_block_ids[i] < 0) throw Err("gs_block_ids: negative block id"); mx = std::max(mx, d.gs_block_ids[i]); }
    b.n = mx + 1;
    b.ptr.assign((size_t)b.n + 1, 0);
    for (int64_t i = 0; i < n; ++i) { b.of[i] = d.gs_block_ids[i]; b.ptr[b.of[i] + 1]++; }
    for (int q = 0; q < b.n; ++q) { if (b.ptr[q + 1] > BB) throw Err("gs_block_ids: a block has more than gs_block_rows rows"); b.ptr[q + 1] += b.ptr[q]; }
    std::vector<int32_t> pos(b.ptr.begin(), b.ptr.end() - 1);
    for (int64_t i = 0; i < n; ++i) { b.lpos[i] = pos[b.of[i]] - b.ptr[b.of[i]]; b.rows[pos[b.of[i]]++] = (int32_t)i; }
  } else {
    b.n = (int)((n + BB - 1) / BB);
    b.ptr.assign((size_t)b.n + 1, 0);
    for (int q = 0; q <= b.n; ++q) b.ptr[q] = (int32_t)std::min<int64_t>(n, (int64_t)q * BB);
    for (int64_t i = 0; i < n; ++i) { b.of[i] = (int32_t)(i / BB); b.lpos[i] = (int32_t)(i % BB); b.rows[i] = (int32_t)i; }
  }
  return b;
}

// block-coloured form: the colour of every sweep block (constant inside a block, coupled blocks differ) as the block colour of
// every row; fills the block lists of g
static std::vector<int32_t> bgsb_block_colours(const amgx_level_desc& d, const SweepBlocks& b, DevBGSB& g) {
  const int64_t n = d.A.n_rows;
  if (d.A.n_cols != n) throw Err("block-coloured Gauss-Seidel: square levels only (rank-partitioned levels sweep in the hybrid form)");
  const int nbc = d.gs_n_block_colors;
  std::vector<int32_t> bcol((size_t)b.n, -1);
  for (int64_t i = 0; i < n; ++i) {
    const int c = d.gs_block_color[i];
    if (c < 0 || c >= nbc) throw Err("gs_block_color: colour out of range");
    if (bcol[b.of[i]] < 0) bcol[b.of[i]] = c;
    else if (bcol[b.of[i]] != c) throw Err("gs_block_color: not constant inside a sweep block");
  }
  std::vector<char> bad(setup_threads(), 0);
  par_for(n, [&](int64_t i0, int64_t i1, int t) {
    for (int64_t i = i0; i < i1; ++i) {
      if (d.color[i] < 0) continue;
      for (int64_t k = d.A.rowptr[i]; k < d.A.rowptr[i + 1]; ++k) {
        const int64_t j = d.A.col[k];
        if (d.color[j] >= 0 && b.of[j] != b.of[i] && bcol[b.of[j]] == bcol[b.of[i]]) { bad[t] = 1; return; }
      }
    }
  });
  for (char c : bad) if (c) throw Err("invalid block colouring: two coupled sweep blocks share a colour (an in-place sweep would race)");
  std::vector<int32_t> list((size_t)b.n);
  g.bc_ptr.assign((size_t)nbc + 1, 0);
  for (int q = 0; q < b.n; ++q) g.bc_ptr[bcol[q] + 1]++;
  for (int c = 0; c < nbc; ++c) g.bc_ptr[c + 1] += g.bc_ptr[c];
  std::vector<int> pos(g.bc_ptr.begin(), g.bc_ptr.end() - 1);
  for (int q = 0; q < b.n; ++q) list[pos[bcol[q]]++] = q;
  g.blk_list.upload(list);
  g.bc = true;
  g.n_bcolors = nbc;
  std::vector<int32_t> of_row((size_t)n);
  for (int64_t i = 0; i < n; ++i) of_row[i] = bcol[b.of[i]];
  return of_row;
}

// fac_k with Dinv_k A_kk = (1 / fac_k) I, fac_k >= 1, on every swept row: the one-pass pre-smoothing from zero is valid where dinv_k
// is a true inverse of fac_k * A_kk (not a pseudo-inverse).  false: some swept row is not of that kind.
static bool bgsb_fac(const amgx_level_desc& d, std::vector<double>& fac) {
  const int64_t n = d.A.n_rows;
  const int bs = d.A.br;
  fac.assign((size_t)n, 1.0);
  std::vector<char> nofac(setup_threads(), 0);
  par_for(n, [&](int64_t i0, int64_t i1, int t) {
    for (int64_t i = i0; i < i1; ++i) {
      if (d.color[i] < 0) continue;
      const double* Akk = nullptr;
      for (int64_t k = d.A.rowptr[i]; k < d.A.rowptr[i + 1]; ++k) if (d.A.col[k] == i) { Akk = d.A.val + k * bs * bs; break; }
      if (!Akk) { nofac[t] = 1; return; }
      const double* Dk = d.dinv + i * bs * bs;
      // M = Dinv_k A_kk must be (1 / fac) I with fac >= 1
      double m00 = 0.0;
      for (int c = 0; c < bs; ++c) m00 += Dk[c] * Akk[c * bs];
      if (!(m00 > 1e-12 && m00 <= 1.0 + 1e-10)) { nofac[t] = 1; return; }
      for (int r = 0; r < bs; ++r)
        for (int c = 0; c < bs; ++c) {
          double m = 0.0;
          for (int q = 0; q < bs; ++q) m += Dk[r * bs + q] * Akk[q * bs + c];
          if (std::fabs(m - (r == c ? m00 : 0.0)) > 1e-10 * m00) { nofac[t] = 1; return; }
        }
      fac[i] = 1.0 / m00;
    }
  });
  for (char c : nofac) if (c) return false;
  return true;
}

// Block-hybrid Gauss-Seidel data of a square-block level (bgsb_sweep_kernel); the blocked colouring is validated (two coupled
// rows of one sweep block sharing a colour would be a data race)
// csr: the level matrix on the device (big levels): the images are then gathered there (devbuild.hpp, dev_build_bsell)
static void build_bgsb(const Knobs& K, const amgx_level_desc& d, DevLevel& L, const DevBcsrSrc* csr = nullptr) {
  const int64_t n = d.A.n_rows;
  const int bs = d.A.br, RB = WAVE / bs;
  DevBGSB& g = L.bgsb;
  const int BB = d.gs_block_rows;
  // ---- validate
  if (bs != 2 && bs != 3 && bs != 6) throw Err("block-hybrid Gauss-Seidel: block sizes 2, 3, 6");
  if (d.A.n_cols < n) throw Err("block-hybrid Gauss-Seidel on block levels: n_cols < n_rows");
  // (n_cols > n_rows: trailing ghost columns of a rank-partitioned level; they belong to no sweep block, so their couplings sit in
  //  `off` / `rest` with global column ids and multiply whatever the caller's exchange left behind the owned entries)
  if (BB < RB || BB > 2048 || (int64_t)2 * BB * bs * 8 > 96 * 1024) throw Err("block-hybrid Gauss-Seidel: gs_block_rows out of range for this block size");
  if (n == 0) { g.BB = BB; return; }
  if (!d.color || d.n_colors <= 0) throw Err("block-hybrid Gauss-Seidel needs a blocked colouring");
  if (!d.dinv) throw Err("dinv missing");
  const int nc = d.n_colors;
  // ---- sweep blocks, and the colouring inside them
  const SweepBlocks b = bgsb_sweep_blocks(d);
  check_colouring(d.A, d.color, nc, [&b](int64_t i, int64_t j) { return b.of[i] == b.of[j]; },
                  d.gs_block_ids ? "invalid blocked colouring: two coupled block rows of one sweep block share a colour"
                                 : "invalid blocked colouring: two coupled block rows of one block share a colour");
  g.BB = BB; g.n_blocks = b.n; g.n_colors = nc;
  // ---- block colours
  std::vector<int32_t> bcolor;
  if (d.gs_block_color && d.gs_n_block_colors > 0) bcolor = bgsb_block_colours(d, b, g);
  // ---- row lists.  off: block by block in list order, every block padded to whole slices
  std::vector<int32_t> rows_off, off_ptr(b.n + 1, 0);
  rows_off.reserve((size_t)n + (size_t)b.n * RB);
  for (int blk = 0; blk < b.n; ++blk) {
    for (int32_t q = b.ptr[blk]; q < b.ptr[blk + 1]; ++q) rows_off.push_back(b.rows[q]);
    while (rows_off.size() % RB) rows_off.push_back(-1);
    off_ptr[blk + 1] = (int32_t)(rows_off.size() / RB);
  }
  // in: per block the swept rows by colour, every (block, colour) group padded to whole slices
  std::vector<int32_t> rows_in, in_ptr((size_t)b.n * nc + 1, 0), in_row;
  for (int blk = 0; blk < b.n; ++blk) {
    for (int c = 0; c < nc; ++c) {
      for (int32_t q = b.ptr[blk]; q < b.ptr[blk + 1]; ++q) if (d.color[b.rows[q]] == c) rows_in.push_back(b.rows[q]);
      while (rows_in.size() % RB) rows_in.push_back(-1);
      in_ptr[(size_t)blk * nc + c + 1] = (int32_t)(rows_in.size() / RB);
    }
  }
  in_row.resize(rows_in.size());
  for (size_t q = 0; q < rows_in.size(); ++q) in_row[q] = rows_in[q] < 0 ? -1 : b.lpos[rows_in[q]];
  // nat: natural order
  std::vector<int32_t> rows_nat((size_t)n);
  for (int64_t i = 0; i < n; ++i) rows_nat[i] = (int32_t)i;
  while (rows_nat.size() % RB) rows_nat.push_back(-1);
  // ---- images: image(rows, sel, out) forms one, on the device where the level matrix is there (the maps and the row list follow
  // it), else by the host loop
  std::vector<double> fac;
  DbBgsbMaps maps{b.of.data(), b.lpos.data(), d.color, nullptr, bcolor.empty() ? nullptr : bcolor.data()};
  struct { DevBuf<int32_t> blk_of, lpos, color, bcolor, rows; DevBuf<double> fac; } dv;
  auto image = [&](const std::vector<int32_t>& rows, int sel, DevMatrix& out) {
    if (csr) {
      auto mirror = [n](auto& buf, const auto* host) { if (host && !buf.p) buf.upload(host, (size_t)n); return buf.p; };
      const DbBgsbMaps dmaps{mirror(dv.blk_of, maps.blk_of), mirror(dv.lpos, maps.lpos), mirror(dv.color, maps.color), mirror(dv.fac, maps.fac),
                             mirror(dv.bcolor, maps.bcolor)};
      dv.rows.upload(rows);
      dev_build_bsell(*csr, dv.rows.p, (int64_t)rows.size(), sel, dmaps, 0, 0.0, out);
    } else build_bsell_sel(d.A, rows, sel, maps, out);
  };
  // Only the in-block couplings to the colours a sweep has ALREADY visited need its new values; everything else -- couplings
  // that leave the block, the diagonal block, in-block couplings to the colours still to come -- multiplies sweep-start values
  // and goes into the streaming phase 0, where all waves work.  The colour phases, which run one after the other inside a
  // workgroup, are left with ~9 % of A for line blocks (22 % for compact blocks) instead of 20 % (50 %).
  image(rows_off, BB_OFF, g.off);
  image(rows_in, BB_IN, g.in);
  image(rows_in, BB_UPIN, g.upin);
  if (g.upin.n_slices != g.in.n_slices) throw Err("block-hybrid Gauss-Seidel: lower / upper slice mismatch");
  g.blk_ptr.upload(b.ptr); g.blk_rows.upload(b.rows);
  g.off_ptr.upload(off_ptr); g.in_ptr.upload(in_ptr); g.in_row.upload(in_row);
  // ---- fac, and the images of the one-pass pre-smoothing from zero
  if (K.bgsb_no_split || !bgsb_fac(d, fac)) return;
  if (g.bc) {
    // block-coloured form: the plain inverse is expected (fac = 1 everywhere), otherwise no split (sweep + full residual).  `offlo`:
    // the entries of `off` that couple to a sweep block a FORWARD sweep has visited; `rest`: those it visits later, and `upin`
    for (int64_t i = 0; i < n; ++i) if (d.color[i] >= 0 && std::fabs(fac[i] - 1.0) > 1e-10) return;
    image(rows_off, BB_OFFLO, g.offlo);
    image(rows_nat, BB_RESTBC, g.rest);
  } else {
    maps.fac = fac.data();
    image(rows_nat, BB_REST, g.rest);
  }
  g.has_split = true;
}

// ---- AMGX_VERIFY_IMAGES: the device-built data against the host builder's, bit by bit.  Both sides evaluate the same rule functions,
// so these checks catch differences of layout and order, not a wrong rule (the oracle comparisons of the test suite do that).

// block-hybrid Gauss-Seidel data of a square-block level
static void verify_bgsb(const Knobs& K, const amgx_level_desc& s, const DevLevel& L) {
  DevLevel H;
  H.n = L.n; H.ncols = L.ncols; H.bs = L.bs;
  build_bgsb(K, s, H, nullptr);
  const DevBGSB &x = L.bgsb, &y = H.bgsb;
  if (x.BB != y.BB || x.n_blocks != y.n_blocks || x.n_colors != y.n_colors || x.has_split != y.has_split) throw Err("AMGX_VERIFY_IMAGES: block-hybrid Gauss-Seidel (blocks): the descriptors differ");
  verify_same_bsell(x.off, y.off, "block-hybrid Gauss-Seidel: off");
  verify_same_bsell(x.in, y.in, "block-hybrid Gauss-Seidel: in");
  verify_same_bsell(x.upin, y.upin, "block-hybrid Gauss-Seidel: upin");
  if (x.has_split) verify_same_bsell(x.rest, y.rest, "block-hybrid Gauss-Seidel: rest");
  if (x.bc != y.bc || x.n_bcolors != y.n_bcolors) throw Err("AMGX_VERIFY_IMAGES: block-coloured Gauss-Seidel: the descriptors differ");
  if (x.bc && x.has_split) verify_same_bsell(x.offlo, y.offlo, "block-coloured Gauss-Seidel: offlo");
}

// ... of a scalar level
static void verify_gsb(const Knobs& K, const amgx_level_desc& s, const DevLevel& L) {
  DevLevel H;
  H.n = L.n; H.ncols = L.ncols; H.bs = L.bs;
  build_gsb(K, s, H, &s.P, nullptr);
  const DevGSB &x = L.gsb, &y = H.gsb;
  if (x.B != y.B || x.G != y.G || x.TH != y.TH || x.n_blocks != y.n_blocks || x.n_colors != y.n_colors || x.lowin_maxw != y.lowin_maxw || x.full_maxw != y.full_maxw ||
      x.has_split != y.has_split) throw Err("AMGX_VERIFY_IMAGES: block-hybrid Gauss-Seidel: the descriptors differ");
  const size_t nsl = (size_t)((int64_t)x.n_blocks * x.B / (WAVE / x.G));
  verify_same_sell(x.full, y.full, nsl, 0, "block-hybrid Gauss-Seidel: A");
  if (x.has_split) {
    verify_same_sell(x.lowin, y.lowin, nsl, 0, "block-hybrid Gauss-Seidel: lower part");
    verify_same_image(x.rest, y.rest, "block-hybrid Gauss-Seidel: rest");
    const auto cx = db_download(x.cvec, (size_t)L.n), cy = db_download(y.cvec, (size_t)L.n);
    if (std::memcmp(cx.data(), cy.data(), (size_t)L.n * sizeof(double)) != 0) throw Err("AMGX_VERIFY_IMAGES: block-hybrid Gauss-Seidel: cvec differs");
  }
}

}  // namespace amgx
