// Kernels of the multi-vector apply path: NV interleaved vectors, entry (row i, column j) at i*NV + j.
// Included ahead of the handle so that Handle::product<NV, EP> (amgx.hip) can name them; the host side is multi.hpp.
//
// The kernels keep the order of additions of their single-vector counterparts per column (pair accumulators, odd trailing
// column last, shuffle reduction), and no operation mixes two columns: a column's result does not depend on its neighbours.
#pragma once

namespace amgx {

constexpr int MULTI_MAX = AMGX_MULTI_MAX;

// NV consecutive doubles at p (16-byte aligned for even NV: interleaved vectors start at 16-byte aligned addresses)
template <int NV>
__device__ __forceinline__ void ldv(const double* __restrict__ p, double (&v)[NV]) {
  if constexpr (NV % 2 == 0) {
    const double2* __restrict__ q = reinterpret_cast<const double2*>(p);
#pragma unroll
    for (int j = 0; j < NV / 2; ++j) { const double2 t = q[j]; v[2 * j] = t.x; v[2 * j + 1] = t.y; }
  } else {
#pragma unroll
    for (int j = 0; j < NV; ++j) v[j] = p[j];
  }
}
template <int NV>
__device__ __forceinline__ void stv(double* __restrict__ p, const double (&v)[NV]) {
  if constexpr (NV % 2 == 0) {
    double2* __restrict__ q = reinterpret_cast<double2*>(p);
#pragma unroll
    for (int j = 0; j < NV / 2; ++j) q[j] = make_double2(v[2 * j], v[2 * j + 1]);
  } else {
#pragma unroll
    for (int j = 0; j < NV; ++j) p[j] = v[j];
  }
}

// epilogue of one row for NV columns; dinv and omega are per row, shared by the columns (arithmetic of store_scalar)
template <int NV, int EP>
__device__ __forceinline__ void store_multi(int64_t row, const double (&acc)[NV], double* y, const EpArgs& ep) {
  double out[NV];
  if constexpr (EP == EP_MULT) {
#pragma unroll
    for (int j = 0; j < NV; ++j) out[j] = acc[j];
  } else if constexpr (EP == EP_RES) {
    double b[NV];
    ldv<NV>(ep.b + row * NV, b);
#pragma unroll
    for (int j = 0; j < NV; ++j) out[j] = b[j] - acc[j];
  } else if constexpr (EP == EP_AXPY) {
    double yin[NV];
    ldv<NV>(ep.yin + row * NV, yin);
#pragma unroll
    for (int j = 0; j < NV; ++j) out[j] = yin[j] + ep.s * acc[j];
  } else if constexpr (EP == EP_JAC) {
    double b[NV], yin[NV];
    ldv<NV>(ep.b + row * NV, b);
    ldv<NV>(ep.yin + row * NV, yin);
    const double d = ep.dinv[row];
#pragma unroll
    for (int j = 0; j < NV; ++j) out[j] = yin[j] + ep.s * (d * (b[j] - acc[j]));
  } else if constexpr (EP == EP_CRES) {
    // y = c .* v - A x (c = ep.dinv per row, v = ep.b interleaved): the residual right after a block-hybrid sweep from zero
    double b[NV];
    ldv<NV>(ep.b + row * NV, b);
    const double d = ep.dinv[row];
#pragma unroll
    for (int j = 0; j < NV; ++j) out[j] = d * b[j] - acc[j];
  } else {
    // store_scalar<EP_CHEB> per column: d, y2 and yin interleaved like y
    static_assert(EP == EP_CHEB, "multi-vector epilogues: MULT, RES, AXPY, JAC, CRES, CHEB");
    double b[NV], yin[NV], dd[NV], dn[NV];
    ldv<NV>(ep.b + row * NV, b);
    ldv<NV>(ep.yin + row * NV, yin);
    if (ep.d) ldv<NV>(ep.d + row * NV, dd);
    else {
#pragma unroll
      for (int j = 0; j < NV; ++j) dd[j] = yin[j];
    }
    const double d = ep.dinv[row];
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      dn[j] = ep.s2 * dd[j] + ep.s * (d * (b[j] - acc[j]));
      out[j] = yin[j] + dn[j];
    }
    if (ep.y2) stv<NV>(ep.y2 + row * NV, dn);
  }
  stv<NV>(y + row * NV, out);
}

// ---- SELL row product for NV interleaved vectors: the batch pipeline of sell_pairs with the gather widened to NV values ----
// XD (the fused down kernel on a diagonal-first image, sell_consume's xd): xd[0 .. NV) receives the x values gathered for entry 0 of
// this lane's row, xd[NV] the matrix value of that entry
template <int K, bool C16, int NV, class V, bool XD = false>
__device__ __forceinline__ void sell_consume_nv(const SellRegs<K, V>& R, const int32_t* __restrict__ cb, int r0, int p,
                                                const double* __restrict__ x, double (&acc0)[NV], double (&acc1)[NV], double* xd = nullptr) {
  double x0[K][NV], x1[K][NV];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int q = p + k;
    const int c0 = C16 ? r0 + cb[2 * q] + (int)(R.ca[k] & 0xffffu) : (int)R.ca[k];
    const int c1 = C16 ? r0 + cb[2 * q + 1] + (int)(R.ca[k] >> 16) : (int)R.cb2[k];
    ldv<NV>(x + (int64_t)c0 * NV, x0[k]);
    ldv<NV>(x + (int64_t)c1 * NV, x1[k]);
  }
  if constexpr (XD) {
    if (p == 0) {
#pragma unroll
      for (int j = 0; j < NV; ++j) xd[j] = x0[0][j];
      xd[NV] = (double)R.v0[0];
    }
  }
#pragma unroll
  for (int k = 0; k < K; ++k) {
#pragma unroll
    for (int j = 0; j < NV; ++j) { acc0[j] += (double)R.v0[k] * x0[k][j]; acc1[j] += (double)R.v1[k] * x1[k][j]; }
  }
}

template <int K, int REM, bool C16, int NV, class V, bool XD = false>
__device__ __forceinline__ void sell_tail_nv(int rem, const SellRegs<K, V>* last, int p_last, const V* __restrict__ vb,
                                             const void* __restrict__ cpv, const int32_t* __restrict__ cb, int r0, int p, int lane,
                                             const double* __restrict__ x, double (&acc0)[NV], double (&acc1)[NV], double* xd = nullptr) {
  if (rem == REM) {
    SellRegs<REM, V> R;
    sell_load<REM, C16>(R, vb, cpv, p, lane);
    if (last) sell_consume_nv<K, C16, NV, V, XD>(*last, cb, r0, p_last, x, acc0, acc1, xd);
    sell_consume_nv<REM, C16, NV, V, XD>(R, cb, r0, p, x, acc0, acc1, xd);
  } else if constexpr (REM > 1) sell_tail_nv<K, REM - 1, C16, NV, V, XD>(rem, last, p_last, vb, cpv, cb, r0, p, lane, x, acc0, acc1, xd);
}

template <bool C16, int NV, class V, int K = SELL_BATCH, bool XD = false>
__device__ __forceinline__ void sell_pairs_nv(int np, const V* __restrict__ vb, const void* __restrict__ cpv, const int32_t* __restrict__ cb,
                                              int r0, int lane, const double* __restrict__ x, double (&acc0)[NV], double (&acc1)[NV],
                                              double* xd = nullptr) {
  const int nfull = np / K, rem = np - nfull * K;
  if (nfull > 0) {
    SellRegs<K, V> A;
    sell_load<K, C16>(A, vb, cpv, 0, lane);
    for (int b = 1; b < nfull; ++b) {
      SellRegs<K, V> B;
      sell_load<K, C16>(B, vb, cpv, b * K, lane);
      sell_consume_nv<K, C16, NV, V, XD>(A, cb, r0, (b - 1) * K, x, acc0, acc1, xd);
      A = B;
    }
    if (K > 1 && rem) sell_tail_nv<K, (K > 1 ? K - 1 : 1), C16, NV, V, XD>(rem, &A, (nfull - 1) * K, vb, cpv, cb, r0, nfull * K, lane, x, acc0, acc1, xd);
    else sell_consume_nv<K, C16, NV, V, XD>(A, cb, r0, (nfull - 1) * K, x, acc0, acc1, xd);
  } else if (K > 1 && rem) sell_tail_nv<K, (K > 1 ? K - 1 : 1), C16, NV, V, XD>(rem, nullptr, 0, vb, cpv, cb, r0, 0, lane, x, acc0, acc1, xd);
}

// acc[j] = (SELL row of the slice with pointers sp0, sp1; this lane) . column j of x          (sell_row_dot_sp for NV vectors)
// XD: xd = NV + 1 doubles of the caller, see sell_consume_nv
// x32 (optional): the interleaved vector that slices in the 32-bit encoding gather from (local-window images: 16-bit slices index the
// NV-wide LDS window x, 32-bit slices -- chunks whose window would not fit -- carry global columns), as in sell_row_dot_sp
template <int NV, class V, bool XD = false>
__device__ __forceinline__ void sell_row_dot_nv_sp(const SellMatT<V>& M, int64_t sp0, int64_t sp1, int lane, int row, const double* __restrict__ x,
                                                   double (&acc)[NV], double* xd = nullptr, const double* __restrict__ x32 = nullptr) {
  const int64_t base = sp0 & ~(int64_t)63;
  const int w = (int)(((sp1 & ~(int64_t)63) - base) >> 6);
  const int np = w >> 1;
  const V* __restrict__ vb = M.val + base;
  double acc0[NV], acc1[NV];
#pragma unroll
  for (int j = 0; j < NV; ++j) { acc0[j] = 0.0; acc1[j] = 0.0; }
  const bool c16 = sp0 & 1;
  const int32_t* __restrict__ cb = M.cbase + (base >> 6);
  const int r0 = (c16 && M.rowrel) ? row : 0;
  V vs = 0;
  int cs = 0;
  if (w & 1) {                                  // odd trailing column: its matrix loads go out first, its gather comes last
    const int64_t o = (int64_t)(w - 1) * WAVE + lane;
    vs = ld_nt(vb + o);
    cs = c16 ? (int)ld_nt(M.col16 + base + o) : ld_nt(M.col32 + base + o);
  }
  const double* __restrict__ xw32 = x32 ? x32 : x;
  if (c16) sell_pairs_nv<true, NV, V, SELL_BATCH, XD>(np, vb, M.col16 + base, cb, r0, lane, x, acc0, acc1, xd);
  else sell_pairs_nv<false, NV, V, SELL_BATCH, XD>(np, vb, M.col32 + base, nullptr, 0, lane, xw32, acc0, acc1, xd);
  if (w & 1) {
    const int c = c16 ? r0 + cb[w - 1] + cs : cs;
    double xs[NV];
    if (c16) ldv<NV>(x + (int64_t)c * NV, xs);             // (two loads, not one through a selected pointer: x may be LDS, xw32 global)
    else ldv<NV>(xw32 + (int64_t)c * NV, xs);
    if constexpr (XD) {
      if (np == 0) {
#pragma unroll
        for (int j = 0; j < NV; ++j) xd[j] = xs[j];
        xd[NV] = (double)vs;
      }
    }
#pragma unroll
    for (int j = 0; j < NV; ++j) acc0[j] += (double)vs * xs[j];
  }
#pragma unroll
  for (int j = 0; j < NV; ++j) acc[j] = acc0[j] + acc1[j];
}
template <int NV, class V>
__device__ __forceinline__ void sell_row_dot_nv(const SellMatT<V>& M, int s, int lane, int row, const double* __restrict__ x, double (&acc)[NV]) {
  sell_row_dot_nv_sp<NV, V>(M, M.slice_ptr[s], M.slice_ptr[s + 1], lane, row, x, acc);
}

// SELL-64-pair, G lanes per row, NV interleaved vectors (sell_spmv_kernel's multi-vector form, same SellMat view)
// V = float: the same kernel on the single-precision image (EP_RES and EP_CHEB are instantiated, as for sell_spmv_kernel)
template <int G, int NV, int EP, class V = double>
__global__ __launch_bounds__(BLOCK) void sell_spmm_kernel(int64_t n_rows, int n_slices, SellMatT<V> M, const double* __restrict__ x, double* y, EpArgs ep) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int s = __builtin_amdgcn_readfirstlane(sell_unit(M) * WAVES_PER_BLOCK + (threadIdx.x >> 6));
  if (s >= n_slices) return;
  const int row = s * (WAVE / G) + lane / G;
  double acc[NV];
  sell_row_dot_nv<NV>(M, s, lane, row, x, acc);
#pragma unroll
  for (int j = 0; j < NV; ++j) {
#pragma unroll
    for (int o = G >> 1; o > 0; o >>= 1) acc[j] += __shfl_xor(acc[j], o, G);
  }
  if ((lane % G) == 0 && row < n_rows) store_multi<NV, EP>(row, acc, y, ep);
}

// windowed SELL (sell_win_spmv_kernel's multi-vector form): the NV row sums go through LDS back to natural order
// V = float: the single-precision image (EP_CRES on `rest` of a scalar Gauss-Seidel level is instantiated)
template <int WB, int NV, int EP, class V = double>
__global__ __launch_bounds__(WB) void sell_win_spmm_kernel(int64_t n_rows, SellMatT<V> M, const uint16_t* __restrict__ rowloc,
                                                           const double* __restrict__ x, double* y, EpArgs ep) {
  __shared__ double buf[WB * NV];
  const int lane = threadIdx.x & (WAVE - 1);
  const int wb = sell_unit(M);
  const int s = __builtin_amdgcn_readfirstlane(wb * (WB / WAVE) + (threadIdx.x >> 6));
  const int64_t slot = (int64_t)s * WAVE + lane;
  const int64_t row = (int64_t)wb * WB + threadIdx.x;
  if (slot < n_rows) {
    double acc[NV];
    sell_row_dot_nv<NV>(M, s, lane, 0, x, acc);
    const int loc = rowloc[slot];
#pragma unroll
    for (int j = 0; j < NV; ++j) buf[loc * NV + j] = acc[j];
  }
  __syncthreads();
  if (row < n_rows) {
    double acc[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) acc[j] = buf[threadIdx.x * NV + j];
    store_multi<NV, EP>(row, acc, y, ep);
  }
}

// ---- the fused down kernels on NV interleaved vectors (AMGX_MULTI_FUSE_DOWN) ---------------------------------
// The single-vector kernels (kernels.hpp: "The fused down kernels") restated column by column: the same image, the same order of
// additions in the row product, the same products and slot sums in the restriction.  r of the chunk's rows sits in LDS interleaved
// (row * NV + column); no operation mixes two columns, every index into an interleaved vector is 64-bit, padding rows and empty
// slices write nothing, and every barrier is reached by every lane (the column loops have compile-time bounds).
//
// ChunkRestrictNV<FB, EPT, NV>: ChunkRestrict for NV columns.  request() is ChunkRestrict::request (nothing it loads is consumed
// before the row product: raw slot pointers).  reduce() runs ChunkRestrict::reduce once per column on the ONE array pr[EPT * FB],
// with a barrier between two columns: LDS stays at 8 * (RPC * NV + EPT * FB) <= 40 KB (three workgroups per CU); holding the
// products of all columns would need 96-112 KB.  The partial sums go to part_nv[dest * NV + column] (R.part), a buffer of the
// multi-vector work space; restrict_sum_nv_kernel adds them.
template <int FB, int EPT, int NV>
struct ChunkRestrictNV {
  int s1, e0, e1, myslot, mydest, pa_raw, pb_raw;
  double wq[EPT];
  int fq[EPT];
  __device__ __forceinline__ void request(int c, const RestrictMat& R) {
    const int s0 = R.chunk_slot[c];
    s1 = R.chunk_slot[c + 1];
    e0 = R.slot_ptr[s0];
    e1 = R.slot_ptr[s1];
#pragma unroll
    for (int q = 0; q < EPT; ++q) {
      const int e = e0 + threadIdx.x + q * FB;
      wq[q] = e < e1 ? ld_nt(R.w + e) : 0.0;
      fq[q] = e < e1 ? (int)ld_nt(R.fi + e) : 0;
    }
    myslot = s0 + threadIdx.x;
    mydest = myslot; pa_raw = 0; pb_raw = 0;
    if (myslot < s1) {
      if (R.dest) mydest = R.dest[myslot];
      pa_raw = R.slot_ptr[myslot];
      pb_raw = R.slot_ptr[myslot + 1];
    }
  }
  // r_lds: r of the chunk's rows, interleaved (the caller's barrier has passed); pr = EPT * FB doubles of LDS
  __device__ __forceinline__ void reduce(const double* r_lds, double* pr, const RestrictMat& R) const {
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      if (j > 0) __syncthreads();                               // the sums of column j - 1 have read pr
#pragma unroll
      for (int q = 0; q < EPT; ++q) {
        const int e = threadIdx.x + q * FB;
        if (e0 + e < e1) pr[e] = wq[q] * r_lds[fq[q] * NV + j];
      }
      __syncthreads();
      if (myslot < s1) {
        const int pa = pa_raw - e0, pb = pb_raw - e0;
        double acc = 0.0;
        for (int k = pa; k < pb; ++k) acc += pr[k];
        R.part[(int64_t)mydest * NV + j] = acc;
      }
      for (int slot = myslot + FB; slot < s1; slot += FB) {     // chunks with more slots than threads
        const int a = R.slot_ptr[slot] - e0, bnd = R.slot_ptr[slot + 1] - e0;
        double acc = 0.0;
        for (int k = a; k < bnd; ++k) acc += pr[k];
        R.part[(int64_t)(R.dest ? R.dest[slot] : slot) * NV + j] = acc;
      }
    }
  }
};

// sell_pre_restrict_kernel<FUSED_BLOCK, MODE, EPT, G, V> on NV interleaved vectors, mode by mode: b (the gathered vector), x and --
// in MODE 2 -- dinv (the right-hand side) are interleaved; dinv of MODE 0 and c of MODE 1 are per row.  The row product is the one of
// sell_spmm_kernel (sell_row_dot_nv_sp, per column the pair order of sell_row_dot_sp and the lane_group_sum<G> tree).
template <int FUSED_BLOCK, int MODE, int EPT, int G, int NV, class V = double>
__global__ __launch_bounds__(FUSED_BLOCK) void sell_pre_restrict_nv_kernel(int64_t n_rows, int chunk0, int n_slices, SellMatT<V> M,
                                                                           const double* __restrict__ b, const double* __restrict__ dinv,
                                                                           double omega, int nt, double* __restrict__ x,
                                                                           const int32_t* __restrict__ chunk_slot,
                                                                           const int32_t* __restrict__ slot_ptr,
                                                                           const double* __restrict__ w, const uint16_t* __restrict__ fi,
                                                                           double* __restrict__ part_nv,
                                                                           const int32_t* __restrict__ dest,
                                                                           const int32_t* __restrict__ slice_list = nullptr) {
  const RestrictMat R{chunk_slot, slot_ptr, w, fi, part_nv, dest};
  constexpr int RPC = FUSED_BLOCK / G;         // rows per chunk
  __shared__ double rl[RPC * NV];
  __shared__ double pr[EPT * FUSED_BLOCK];
  const int lane = threadIdx.x & (WAVE - 1);
  const int c = chunk0 + sell_unit(M);
  const int sq = c * (FUSED_BLOCK / WAVE) + (threadIdx.x >> 6);
  const int s_raw = slice_list ? slice_list[sq] : sq;          // compact chunks: as in the single-vector kernel
  const int s = __builtin_amdgcn_readfirstlane(s_raw < 0 ? n_slices : s_raw);
  const int row = s * (WAVE / G) + lane / G;
  const int lrow = (threadIdx.x >> 6) * (WAVE / G) + lane / G;     // row inside the chunk
  const bool writer = (lane % G) == 0;
  const bool has_slice = s < n_slices;
  const int64_t sp0 = has_slice ? M.slice_ptr[s] : 0, sp1 = has_slice ? M.slice_ptr[s + 1] : 0;
  ChunkRestrictNV<FUSED_BLOCK, EPT, NV> cr;
  cr.request(c, R);
  double r[NV];
#pragma unroll
  for (int j = 0; j < NV; ++j) r[j] = 0.0;
  if (s < n_slices) {
    // own-row operands ahead of the row product, as in the single-vector kernel; dv: the right-hand side of MODE 2
    double bi[NV], dv[NV], di = 0.0;
#pragma unroll
    for (int j = 0; j < NV; ++j) { bi[j] = 0.0; dv[j] = 0.0; }
    const int64_t io = (int64_t)row * NV;
    constexpr bool XD = MODE == 0 && G == 1;
    const bool wdiag = XD && M.wdiag && M.diag_first;
    const bool hoist = MODE != 0 || G > 1 || (nt & EPF_HOIST);
    if (!wdiag && hoist && writer && row < n_rows) {
      if (MODE != 2) ldv<NV>(b + io, bi);
      if (MODE == 2) ldv<NV>(dinv + io, dv);
      else di = (MODE != 1 && (nt & EPF_NT)) ? ld_nt(dinv + row) : dinv[row];
    }
    double acc[NV], xd[NV + 1];
#pragma unroll
    for (int j = 0; j <= NV; ++j) xd[j] = 0.0;
    sell_row_dot_nv_sp<NV, V, XD>(M, sp0, sp1, lane, row, b, acc, xd);
#pragma unroll
    for (int j = 0; j < NV; ++j) acc[j] = lane_group_sum<G>(acc[j]);
    if (writer && row < n_rows) {
      if (MODE == 1) {
#pragma unroll
        for (int j = 0; j < NV; ++j) r[j] = di * bi[j] - acc[j];
      } else if (MODE == 2) {
#pragma unroll
        for (int j = 0; j < NV; ++j) r[j] = dv[j] - acc[j];
      } else {
        if (wdiag) {
          const double wd = xd[NV];
#pragma unroll
          for (int j = 0; j < NV; ++j) {
            bi[j] = xd[j];
            acc[j] = acc[j] - wd * bi[j] + (wd != 0.0 ? omega * bi[j] : 0.0);
          }
          di = wd / omega;
        } else if (!hoist) { ldv<NV>(b + io, bi); di = (nt & EPF_NT) ? ld_nt(dinv + row) : dinv[row]; }
        double xi[NV];
#pragma unroll
        for (int j = 0; j < NV; ++j) {
          r[j] = bi[j] - acc[j];
          xi[j] = omega * (di * bi[j]);                        // jacobi_down_store per column
          if (nt & EPF_FOLD) xi[j] += omega * (di * r[j]);
        }
        if (nt & EPF_NT) {
#pragma unroll
          for (int j = 0; j < NV; ++j) __builtin_nontemporal_store(xi[j], x + io + j);
        } else stv<NV>(x + io, xi);
      }
    }
  }
  if (writer) {
#pragma unroll
    for (int j = 0; j < NV; ++j) rl[lrow * NV + j] = r[j];
  }
  __syncthreads();
  cr.reduce(rl, pr, R);
}

// sell_win_pre_restrict_kernel<WB, EPT, 1> on NV interleaved vectors: the residual after a block-hybrid sweep from zero on the
// windowed image of A_rest, r = c .* x - A_rest x (b = the swept x, interleaved; dinv = c per row), row sums through LDS back to
// natural order as in sell_win_spmm_kernel.  (MODE 0 of the windowed family is the AMGX_APRE_WINDOW A/B hook: not built.)
// V = float: the single-precision image of a windowed `rest` (AMGX_MULTI_FUSE_DOWN_F32)
template <int WB, int EPT, int MODE, int NV, class V = double>
__global__ __launch_bounds__(WB) void sell_win_pre_restrict_nv_kernel(int64_t n_rows, int win0, SellMatT<V> M, const uint16_t* __restrict__ rowloc,
                                                                      const double* __restrict__ b, const double* __restrict__ dinv,
                                                                      RestrictMat R) {
  static_assert(MODE == 1, "the windowed multi-vector down kernel is built for MODE 1 alone");
  __shared__ double buf[WB * NV];
  __shared__ double pr[EPT * WB];
  const int lane = threadIdx.x & (WAVE - 1);
  const int c = win0 + sell_unit(M);
  const int s = __builtin_amdgcn_readfirstlane(c * (WB / WAVE) + (threadIdx.x >> 6));
  const int64_t slot = (int64_t)s * WAVE + lane;
  const int64_t row = (int64_t)c * WB + threadIdx.x;
  ChunkRestrictNV<WB, EPT, NV> cr;
  cr.request(c, R);
  double bi[NV], di = 0.0;
#pragma unroll
  for (int j = 0; j < NV; ++j) bi[j] = 0.0;
  if (row < n_rows) { ldv<NV>(b + row * NV, bi); di = dinv[row]; }
  if (slot < n_rows) {
    double acc[NV];
    sell_row_dot_nv<NV>(M, s, lane, 0, b, acc);
    const int loc = rowloc[slot];
#pragma unroll
    for (int j = 0; j < NV; ++j) buf[loc * NV + j] = acc[j];
  }
  __syncthreads();
  double r[NV];
#pragma unroll
  for (int j = 0; j < NV; ++j) r[j] = row < n_rows ? di * bi[j] - buf[threadIdx.x * NV + j] : 0.0;
#pragma unroll
  for (int j = 0; j < NV; ++j) buf[threadIdx.x * NV + j] = r[j];      // (same thread, same entries: the residuals replace the row sums)
  __syncthreads();
  cr.reduce(buf, pr, R);
}

// LdsWindow for NV interleaved vectors: xw[k * NV + j] = src[ccol[k0 + k] * NV + j] for the listed columns of unit c.  request()
// issues the NV-wide loads into registers and consumes nothing, publish() writes them to LDS (every thread takes part, the caller's
// barrier follows).  wcap: the doubles-per-column capacity of the caller's window (the longest list of the level, DownPlan::lw_max_list):
// no list is longer, the bound only keeps a damaged list from writing past the window.
template <int CAP, int TB, int NV>
struct LdsWindowNV {
  static constexpr int NQ = (CAP + TB - 1) / TB;
  int k0, k1;
  double xv[NQ][NV];
  __device__ __forceinline__ void request(int c, int wcap, const int32_t* __restrict__ cptr, const int32_t* __restrict__ ccol, const double* __restrict__ src) {
    k0 = cptr[c]; k1 = cptr[c + 1];
    if (k1 - k0 > wcap) k1 = k0 + wcap;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int k = k0 + threadIdx.x + q * TB;
#pragma unroll
      for (int j = 0; j < NV; ++j) xv[q][j] = 0.0;
      if (k < k1) ldv<NV>(src + (int64_t)ccol[k] * NV, xv[q]);
    }
  }
  __device__ __forceinline__ void publish(double* xw) const {
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int k = threadIdx.x + q * TB;
      if (k0 + k < k1) stv<NV>(xw + k * NV, xv[q]);
    }
  }
};

// sell_lw_pre_restrict_kernel<EPT, G, 1, V> on NV interleaved vectors (AMGX_MULTI_FUSE_DOWN_F32): the residual after a
// block-hybrid sweep from zero on the local-window image of A_rest, r = c .* x - A_rest x (b = the swept x, interleaved; dinv = c per
// row).  The window holds the chunk's listed columns of x for all NV columns, staged once; 16-bit slices gather NV-wide from it,
// 32-bit slices (chunks beyond the capacity) from global memory.  Per column the pair order of sell_row_dot_sp and the tree of
// lane_group_sum<G>.  Dynamic LDS (down_nv_lw_lds_bytes, down_plan.hpp): [wcap * NV] the window | [512 / G * NV] r | [EPT * 512] the
// products of one column at a time.  V = float: the single-precision image; the AMGX_GS_F32_WIDE twin runs V = double on its rounded
// values.  (MODE 0 of the family, the Jacobi pass on A', is not built.)
template <int EPT, int G, int MODE, int NV, class V = double>
__global__ __launch_bounds__(512) void sell_lw_pre_restrict_nv_kernel(int64_t n_rows, int n_slices, SellMatT<V> M, int wcap,
                                                                      const int32_t* __restrict__ lw_cptr, const int32_t* __restrict__ lw_ccol,
                                                                      const double* __restrict__ b, const double* __restrict__ dinv,
                                                                      const int32_t* __restrict__ chunk_slot, const int32_t* __restrict__ slot_ptr,
                                                                      const double* __restrict__ w, const uint16_t* __restrict__ fi,
                                                                      double* __restrict__ part_nv, const int32_t* __restrict__ dest) {
  static_assert(MODE == 1, "the local-window multi-vector down kernel is built for MODE 1 alone");
  constexpr int FB = 512;
  constexpr int ROWS = FB / G;
  const RestrictMat R{chunk_slot, slot_ptr, w, fi, part_nv, dest};
  extern __shared__ __attribute__((aligned(16))) double lw_nv_lds[];
  double* const xw = lw_nv_lds;
  double* const rl = xw + (int64_t)wcap * NV;
  double* const pr = rl + ROWS * NV;
  const int lane = threadIdx.x & (WAVE - 1);
  const int c = sell_unit(M);
  const int s = __builtin_amdgcn_readfirstlane(c * (FB / WAVE) + (threadIdx.x >> 6));
  const int row = s * (WAVE / G) + lane / G;
  const int lrow = (threadIdx.x >> 6) * (WAVE / G) + lane / G;
  const bool writer = (lane % G) == 0;
  // the window and the restriction data: all loads of the prologue are requested before anything is consumed
  LdsWindowNV<LW_CAP, FB, NV> win;
  win.request(c, wcap, lw_cptr, lw_ccol, b);
  const bool has_slice = s < n_slices;
  const int64_t sp0 = has_slice ? M.slice_ptr[s] : 0, sp1 = has_slice ? M.slice_ptr[s + 1] : 0;
  ChunkRestrictNV<FB, EPT, NV> cr;
  cr.request(c, R);
  double bi[NV], di = 0.0;
#pragma unroll
  for (int j = 0; j < NV; ++j) bi[j] = 0.0;
  if (writer && has_slice && row < n_rows) { ldv<NV>(b + (int64_t)row * NV, bi); di = dinv[row]; }
  win.publish(xw);
  __syncthreads();
  double r[NV];
#pragma unroll
  for (int j = 0; j < NV; ++j) r[j] = 0.0;
  if (has_slice) {
    double acc[NV];
    sell_row_dot_nv_sp<NV, V>(M, sp0, sp1, lane, 0, xw, acc, nullptr, b);   // 16-bit slices: indices into the window; 32-bit: global columns
#pragma unroll
    for (int j = 0; j < NV; ++j) acc[j] = lane_group_sum<G>(acc[j]);
    if (writer && row < n_rows) {
#pragma unroll
      for (int j = 0; j < NV; ++j) r[j] = di * bi[j] - acc[j];
    }
  }
  if (writer) {
#pragma unroll
    for (int j = 0; j < NV; ++j) rl[lrow * NV + j] = r[j];
  }
  __syncthreads();
  cr.reduce(rl, pr, R);
}

// ---- the diagonal-image down kernels on NV interleaved vectors (AMGX_MULTI_FUSE_DOWN_DIA) ----------------------
// dia_pre_restrict_kernel<K, EPT> on interleaved b and x.  The matrix values U_k[row], U_k[row - o_k] and dinv of the row and of its
// 2K neighbours are loaded once per row; b of the own row and of the neighbours per column.  Per column the expressions and their
// order are the single-vector kernel's: lower couplings in descending k, the diagonal term omega * b_i where dinv_i != 0, upper
// couplings in ascending k, x_j = omega * (dinv_j * b_j) for the neighbours, the Jacobi store with and without EPF_FOLD / EPF_NT.
// b of the own row is loaded, and x stored, NV wide.  The neighbours' b are requested and consumed dia_nv_cols(K, NV) columns at a
// time: all operands of four columns at K = 7 are 29 matrix / dinv values + 60 b values, and the compiler requests whatever it sees
// (195-212 VGPRs, one workgroup per CU).  The passes are therefore kept apart by an opaque copy of the row index, from which the
// 2K addresses of a pass are formed again instead of being held across all passes: two columns per pass (16-byte loads) up to
// K = 5, one from K = 6 on -- what stays near the 128 VGPRs of two workgroups per CU, where the single-vector kernel runs.
// A column's own sequence of operations does not change.
constexpr int DIA_NV_PAIR_MAX_K = 5;
constexpr int dia_nv_cols(int K, int NV) { return K <= DIA_NV_PAIR_MAX_K && NV >= 2 ? 2 : 1; }
template <int K, int EPT, int NV>
__global__ __launch_bounds__(512) void dia_pre_restrict_nv_kernel(int n_rows, int n_slices, DiaMat D, const double* __restrict__ b,
                                                                  const double* __restrict__ dinv, double omega, int nt, double* __restrict__ x,
                                                                  const int32_t* __restrict__ chunk_slot, const int32_t* __restrict__ slot_ptr,
                                                                  const double* __restrict__ w, const uint16_t* __restrict__ fi,
                                                                  double* __restrict__ part_nv, const int32_t* __restrict__ dest,
                                                                  const int32_t* __restrict__ slice_list) {
  constexpr int FB = 512, HC = dia_nv_cols(K, NV);
  static_assert(NV % HC == 0, "the columns are taken HC at a time");
  const RestrictMat R{chunk_slot, slot_ptr, w, fi, part_nv, dest};
  __shared__ double rl[FB * NV];
  __shared__ double pr[EPT * FB];
  const int lane = threadIdx.x & (WAVE - 1);
  const int c = D.xcd ? xcd_remap((int)blockIdx.x, (int)gridDim.x) : (int)blockIdx.x;
  const int sq = c * (FB / WAVE) + (threadIdx.x >> 6);
  const int s_raw = slice_list ? slice_list[sq] : sq;          // compact chunks: as in the single-vector kernel
  const int s = __builtin_amdgcn_readfirstlane(s_raw < 0 ? n_slices : s_raw);
  const int row = s * WAVE + lane;
  ChunkRestrictNV<FB, EPT, NV> cr;
  cr.request(c, R);                            // chunk-local restriction data first (nothing of it is consumed before the row product)
  double* const rrow = rl + threadIdx.x * NV;  // r of this lane's row, all columns
  if (s < n_slices && row < n_rows) {
    // per row: the matrix values and dinv (out-of-range neighbours read row i itself and are masked)
    double al[K], au[K], dl[K], du[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const double* __restrict__ U = D.val + (int64_t)k * n_rows;
      const int o = D.off[k];
      const int jl = row - o >= 0 ? row - o : row;
      const int ju = row + o < n_rows ? row + o : row;
      al[k] = U[jl]; dl[k] = dinv[jl];
      au[k] = U[row]; du[k] = dinv[ju];
    }
    const double di = dinv[row];
    const int64_t io = (int64_t)row * NV;
    double bi[NV], xi[NV];
    ldv<NV>(b + io, bi);
#pragma unroll
    for (int h = 0; h < NV; h += HC) {
      // per pass: every operand requested before the first product
      double bl[K][HC], bu[K][HC];
      int rw = row;                              // (opaque per pass: the pass requests nothing before the pass ahead of it has been consumed)
      asm volatile("" : "+v"(rw));
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const int o = D.off[k];
        const int jl = rw - o >= 0 ? rw - o : rw;
        const int ju = rw + o < n_rows ? rw + o : rw;
        ldv<HC>(b + (int64_t)jl * NV + h, bl[k]);
        ldv<HC>(b + (int64_t)ju * NV + h, bu[k]);
      }
#pragma unroll
      for (int j = 0; j < HC; ++j) {
        double acc = 0.0;
#pragma unroll
        for (int k = K - 1; k >= 0; --k)
          if (row - D.off[k] >= 0) acc += al[k] * (omega * (dl[k] * bl[k][j]));
        if (di != 0.0) acc += omega * bi[h + j];
#pragma unroll
        for (int k = 0; k < K; ++k)
          if (row + D.off[k] < n_rows) acc += au[k] * (omega * (du[k] * bu[k][j]));
        const double r = bi[h + j] - acc;
        xi[h + j] = omega * (di * bi[h + j]);
        if (nt & EPF_FOLD) xi[h + j] += omega * (di * r);
        rrow[h + j] = r;
      }
    }
    if (nt & EPF_NT) {
#pragma unroll
      for (int j = 0; j < NV; ++j) __builtin_nontemporal_store(xi[j], x + io + j);
    } else stv<NV>(x + io, xi);
  } else {
#pragma unroll
    for (int j = 0; j < NV; ++j) rrow[j] = 0.0;                // padding rows and empty slices: r = 0, nothing written to x
  }
  __syncthreads();
  cr.reduce(rl, pr, R);
}

// dia_box_pre_restrict_kernel<K> on interleaved vectors: the same dia::BoxGrid arithmetic, up to 4 rows per lane.  The workgroup
// publishes xs[local * NV + j] = omega * (dinv * b_j) of its rows for all columns first; a row then takes, per column, its in-box
// neighbours from xs and the others from b_j and dinv as the single-vector kernel does (columns dia_nv_cols(K, NV) at a time, see above);
// r goes to rl[local * NV + j].  After the barrier the restriction runs ONE column at a time on the one product array that aliases
// xs: per column the request / products passes of four entries per lane and the slot sums in the single-vector kernel's order, with
// a barrier between two columns.  w and fi are read again per column (they hit the L2 after the first): holding a box's 13 entries
// per lane at cfg 2 in registers across the row products is what the single-vector kernel avoids, too.
// LDS (dynamic, down_nv_dia_lds_bytes): r [lds_rows * NV], then x_j [lds_rows * NV] / the products of one column [most entries of a box].
template <int K, int NV>
__global__ __launch_bounds__(512, (NV > 2 ? 2 : 4)) void dia_box_pre_restrict_nv_kernel(int n_rows, DiaMat D, dia::BoxGrid G, int lds_rows,
                                                                      const double* __restrict__ b, const double* __restrict__ dinv,
                                                                      double omega, int nt, double* __restrict__ x,
                                                                      const int32_t* __restrict__ chunk_slot, const int32_t* __restrict__ slot_ptr,
                                                                      const double* __restrict__ w, const uint16_t* __restrict__ fi,
                                                                      double* __restrict__ part_nv, const int32_t* __restrict__ dest) {
  constexpr int FB = 512, RPT = dia::BOX_MAX_ROWS / FB, EB = 4, HC = dia_nv_cols(K, NV);
  static_assert(NV % HC == 0, "the columns are taken HC at a time");
  extern __shared__ double box_nv_lds[];
  double* rl = box_nv_lds;
  double* xs = box_nv_lds + (size_t)lds_rows * NV;
  double* pr = xs;
  const int c = (int)blockIdx.x;
  const dia::BoxAt at = dia::box_at(G, c);
  const int nrow = dia::box_nrows(G, at);
  const int s0 = chunk_slot[c], s1 = chunk_slot[c + 1];
  const int e0 = slot_ptr[s0], e1 = slot_ptr[s1];
  // publish x_j of the box's rows, all columns
#pragma unroll
  for (int j = 0; j < RPT; ++j) {
    const int local = (int)threadIdx.x + j * FB;
    if (local < nrow) {
      const int row = dia::box_global(G, at, dia::box_row(G, at, local));
      double bq[NV];
      ldv<NV>(b + (int64_t)row * NV, bq);
      const double dq = dinv[row];
#pragma unroll
      for (int q = 0; q < NV; ++q) xs[local * NV + q] = omega * (dq * bq[q]);
    }
  }
  __syncthreads();
#pragma unroll 1
  for (int local = (int)threadIdx.x; local < nrow; local += FB) {
    const dia::BoxRow br = dia::box_row(G, at, local);
    const int row = dia::box_global(G, at, br);
    // per row: the matrix values, and dinv of the out-of-box neighbours (out-of-range neighbours read row i itself and are masked)
    double al[K], au[K], dl[K], du[K];
    bool inl[K], inu[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const double* __restrict__ U = D.val + (int64_t)k * n_rows;
      const int o = D.off[k];
      const int jl = row - o >= 0 ? row - o : row;
      const int ju = row + o < n_rows ? row + o : row;
      inl[k] = dia::box_has(G, at, br, k, false);
      inu[k] = dia::box_has(G, at, br, k, true);
      al[k] = U[jl]; au[k] = U[row];
      dl[k] = 0.0; du[k] = 0.0;
      if (!inl[k]) dl[k] = dinv[jl];
      if (!inu[k]) du[k] = dinv[ju];
    }
    const double di = dinv[row];
    const int64_t io = (int64_t)row * NV;
    double bi[NV], xi[NV];
    ldv<NV>(b + io, bi);
#pragma unroll
    for (int h = 0; h < NV; h += HC) {
      double bl[K][HC], bu[K][HC];
      int rw = row;                              // (opaque per pass: the pass requests nothing before the pass ahead of it has been consumed)
      asm volatile("" : "+v"(rw));
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const int o = D.off[k];
        const int jl = rw - o >= 0 ? rw - o : rw;
        const int ju = rw + o < n_rows ? rw + o : rw;
#pragma unroll
        for (int j = 0; j < HC; ++j) { bl[k][j] = 0.0; bu[k][j] = 0.0; }
        if (!inl[k]) ldv<HC>(b + (int64_t)jl * NV + h, bl[k]);
        if (!inu[k]) ldv<HC>(b + (int64_t)ju * NV + h, bu[k]);
      }
#pragma unroll
      for (int j = 0; j < HC; ++j) {
        const int q = h + j;
        double acc = 0.0;
#pragma unroll
        for (int k = K - 1; k >= 0; --k)
          if (row - D.off[k] >= 0) {
            const double xj = inl[k] ? xs[(local - dia::box_local_offset(G, at, k)) * NV + q] : omega * (dl[k] * bl[k][j]);
            acc += al[k] * xj;
          }
        if (di != 0.0) acc += omega * bi[q];
#pragma unroll
        for (int k = 0; k < K; ++k)
          if (row + D.off[k] < n_rows) {
            const double xj = inu[k] ? xs[(local + dia::box_local_offset(G, at, k)) * NV + q] : omega * (du[k] * bu[k][j]);
            acc += au[k] * xj;
          }
        const double rj = bi[q] - acc;
        xi[q] = omega * (di * bi[q]);
        if (nt & EPF_FOLD) xi[q] += omega * (di * rj);
        rl[local * NV + q] = rj;
      }
    }
    if (nt & EPF_NT) {
#pragma unroll
      for (int j = 0; j < NV; ++j) __builtin_nontemporal_store(xi[j], x + io + j);
    } else stv<NV>(x + io, xi);
  }
  // chunk-local restriction, column by column: part_nv[slot * NV + j] = sum over the slot's entries of w * r_lds[fi * NV + j]
  double wq[EB];
  int fq[EB];
  auto request = [&](int eb) {
#pragma unroll
    for (int q = 0; q < EB; ++q) {
      const int e = eb + q * FB;
      wq[q] = e < e1 ? ld_nt(w + e) : 0.0;
      fq[q] = e < e1 ? (int)ld_nt(fi + e) : 0;
    }
  };
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    auto products = [&](int eb) {
#pragma unroll
      for (int q = 0; q < EB; ++q) {
        const int e = eb + q * FB;
        if (e < e1) pr[e - e0] = wq[q] * rl[fq[q] * NV + j];
      }
    };
    int eb = e0 + (int)threadIdx.x;
    request(eb);
    __syncthreads();                             // column 0: r of the box is complete, x_j no longer read; later: the sums of column j - 1 have read pr
    products(eb);
    for (eb += EB * FB; eb < e1; eb += EB * FB) { request(eb); products(eb); }
    __syncthreads();
    for (int slot = s0 + (int)threadIdx.x; slot < s1; slot += FB) {
      const int a = slot_ptr[slot] - e0, bnd = slot_ptr[slot + 1] - e0;
      double acc = 0.0;
      for (int k = a; k < bnd; ++k) acc += pr[k];
      part_nv[(int64_t)(dest ? dest[slot] : slot) * NV + j] = acc;
    }
  }
}

// restrict_sum_kernel on the interleaved partial sums part_nv[slot * NV + column]: per column the same optr / oidx order, the same
// first-two-then-rest additions and the same shuffle tree; RSUM_R coarse rows per lane group
template <int NV>
__global__ __launch_bounds__(BLOCK) void restrict_sum_nv_kernel(int64_t n_coarse, const int32_t* __restrict__ optr,
                                                                const int32_t* __restrict__ oidx,
                                                                const double* __restrict__ part, double* __restrict__ bc) {
  const int64_t t = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  const int64_t J0 = (t / RSUM_G) * RSUM_R;
  const int sub = (int)(t % RSUM_G);
  int kb[RSUM_R], ke[RSUM_R];
#pragma unroll
  for (int r = 0; r < RSUM_R; ++r) {
    const int64_t J = J0 + r;
    kb[r] = J < n_coarse ? optr[J] + sub : 0;
    ke[r] = J < n_coarse ? optr[J + 1] : 0;
  }
  double acc[RSUM_R][NV];
  if (oidx) {
    int i0[RSUM_R], i1[RSUM_R];
#pragma unroll
    for (int r = 0; r < RSUM_R; ++r) {
      i0[r] = kb[r] < ke[r] ? oidx[kb[r]] : -1;
      i1[r] = kb[r] + RSUM_G < ke[r] ? oidx[kb[r] + RSUM_G] : -1;
    }
#pragma unroll
    for (int r = 0; r < RSUM_R; ++r) {
      double p0[NV], p1[NV];
#pragma unroll
      for (int j = 0; j < NV; ++j) { p0[j] = 0.0; p1[j] = 0.0; }
      if (i0[r] >= 0) ldv<NV>(part + (int64_t)i0[r] * NV, p0);
      if (i1[r] >= 0) ldv<NV>(part + (int64_t)i1[r] * NV, p1);
#pragma unroll
      for (int j = 0; j < NV; ++j) acc[r][j] = p0[j] + p1[j];
    }
#pragma unroll
    for (int r = 0; r < RSUM_R; ++r)
      for (int k = kb[r] + 2 * RSUM_G; k < ke[r]; k += RSUM_G) {
        double p[NV];
        ldv<NV>(part + (int64_t)oidx[k] * NV, p);
#pragma unroll
        for (int j = 0; j < NV; ++j) acc[r][j] += p[j];
      }
  } else {
#pragma unroll
    for (int r = 0; r < RSUM_R; ++r) {
#pragma unroll
      for (int j = 0; j < NV; ++j) acc[r][j] = 0.0;
      for (int k = kb[r]; k < ke[r]; k += RSUM_G) {            // partials stored row by row (dest)
        double p[NV];
        ldv<NV>(part + (int64_t)k * NV, p);
#pragma unroll
        for (int j = 0; j < NV; ++j) acc[r][j] += p[j];
      }
    }
  }
#pragma unroll
  for (int r = 0; r < RSUM_R; ++r) {
#pragma unroll
    for (int j = 0; j < NV; ++j) {
#pragma unroll
      for (int o = RSUM_G >> 1; o > 0; o >>= 1) acc[r][j] += __shfl_xor(acc[r][j], o, RSUM_G);
    }
    if (J0 + r < n_coarse && sub == 0) stv<NV>(bc + (J0 + r) * NV, acc[r]);
  }
}

// CSR-vector, G lanes per row, NV interleaved vectors (csrvec_spmv_kernel's multi-vector form)
template <int G, int NV, int EP>
__global__ __launch_bounds__(BLOCK) void csrvec_spmm_kernel(int64_t n_rows, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ cols,
                                                            const double* __restrict__ vals, const double* __restrict__ x, double* y, EpArgs ep) {
  const int64_t t = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  const int64_t row = t / G;
  const int sub = (int)(t % G);
  double acc[NV];
#pragma unroll
  for (int j = 0; j < NV; ++j) acc[j] = 0.0;
  if (row < n_rows) {
    const int e = rowptr[row + 1];
    for (int k = rowptr[row] + sub; k < e; k += G) {
      const double v = vals[k];
      double xv[NV];
      ldv<NV>(x + (int64_t)cols[k] * NV, xv);
#pragma unroll
      for (int j = 0; j < NV; ++j) acc[j] += v * xv[j];
    }
  }
#pragma unroll
  for (int j = 0; j < NV; ++j) {
#pragma unroll
    for (int o = G >> 1; o > 0; o >>= 1) acc[j] += __shfl_xor(acc[j], o, G);
  }
  if (row < n_rows && sub == 0) store_multi<NV, EP>(row, acc, y, ep);
}

// ---- block levels (AMGX_MULTI_FUSE): a gathered block column is BS*NV contiguous doubles ---------------------
// Epilogue of the kernels that hold ONE LANE PER SCALAR ROW (lane r of the BS lanes from `base` on owns row r of block row brow):
// per column the arithmetic of bsell_spmv_kernel's epilogue -- t = b - acc exchanged over the block row, u = Dinv_row . t.
// Every lane of the wave calls it (the exchange is a wave operation); only `writer` lanes touch memory.
template <int BS, int NV, int EP>
__device__ __forceinline__ void block_row_epilogue_nv(bool writer, int64_t brow, int r, int base, const double (&acc)[NV], double* y, const EpArgs& ep) {
  const int64_t io = (brow * BS + r) * NV;
  double out[NV];
  if constexpr (EP == EP_JAC || EP == EP_CHEB) {
    double t[NV], yin[NV], u[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) { t[j] = 0.0; yin[j] = 0.0; u[j] = 0.0; }
    if (writer) {
      double b[NV];
      ldv<NV>(ep.b + io, b);
      ldv<NV>(ep.yin + io, yin);
#pragma unroll
      for (int j = 0; j < NV; ++j) t[j] = b[j] - acc[j];
    }
#pragma unroll
    for (int c = 0; c < BS; ++c) {
      const double dc = writer ? ep.dinv[brow * (BS * BS) + r * BS + c] : 0.0;
#pragma unroll
      for (int j = 0; j < NV; ++j) {
        const double tc = __shfl(t[j], base + c, WAVE);
        u[j] += dc * tc;
      }
    }
    if (!writer) return;
    if constexpr (EP == EP_CHEB) {
      double dd[NV], dn[NV];
      if (ep.d) ldv<NV>(ep.d + io, dd);
      else {
#pragma unroll
        for (int j = 0; j < NV; ++j) dd[j] = yin[j];
      }
#pragma unroll
      for (int j = 0; j < NV; ++j) {
        dn[j] = ep.s2 * dd[j] + ep.s * u[j];
        out[j] = yin[j] + dn[j];
      }
      if (ep.y2) stv<NV>(ep.y2 + io, dn);
    } else {
#pragma unroll
      for (int j = 0; j < NV; ++j) out[j] = yin[j] + ep.s * u[j];
    }
  } else {
    if (!writer) return;
    if constexpr (EP == EP_MULT) {
#pragma unroll
      for (int j = 0; j < NV; ++j) out[j] = acc[j];
    } else if constexpr (EP == EP_RES) {
      double b[NV];
      ldv<NV>(ep.b + io, b);
#pragma unroll
      for (int j = 0; j < NV; ++j) out[j] = b[j] - acc[j];
    } else {
      static_assert(EP == EP_AXPY, "multi-vector block epilogues: MULT, RES, AXPY, JAC, CHEB");
      double yin[NV];
      ldv<NV>(ep.yin + io, yin);
#pragma unroll
      for (int j = 0; j < NV; ++j) out[j] = yin[j] + ep.s * acc[j];
    }
  }
  stv<NV>(y + io, out);
}

// BSELL, one lane per scalar row, NV interleaved vectors (bsell_spmv_kernel's multi-vector form, same BSellMatT view).  Per block
// step: the value loads of bsell_block_step (pair order, odd trailing column last) and ONE gather of the block's BS*NV doubles.
// Only the plain row loop: BSellMat::xmode (AMGX_BSELL_XMODE) is ignored here -- its variants rearrange the BS 8-byte gathers of the
// single-vector kernel, which do not exist in this one.
// V = float: the single-precision image (EP_RES and EP_CHEB are instantiated)
template <int BS, int NV, int EP, class V = double>
__global__ __launch_bounds__(BLOCK) void bsell_spmm_kernel(int64_t n_rows, int n_slices, BSellMatT<V> M, const double* __restrict__ x, double* y, EpArgs ep) {
  constexpr int RB = WAVE / BS;
  const int lane = threadIdx.x & (WAVE - 1);
  const int s = __builtin_amdgcn_readfirstlane(blockIdx.x * WAVES_PER_BLOCK + (threadIdx.x >> 6));
  if (s >= n_slices) return;
  const int rbl = lane / BS < RB ? lane / BS : RB - 1;      // idle lanes (lane >= RB*BS) shadow the last block row
  const int r = lane % BS;
  const int64_t brow = (int64_t)s * RB + rbl;
  const bool active = lane < RB * BS && brow < n_rows;
  const int64_t k0 = M.slice_ptr[s];
  const int w = (int)(M.slice_ptr[s + 1] - k0);
  const V* __restrict__ vb = M.val + k0 * (BS * WAVE);
  const int32_t* __restrict__ cb = M.col + k0 * RB;
  double acc[NV];
#pragma unroll
  for (int j = 0; j < NV; ++j) acc[j] = 0.0;
  for (int k = 0; k < w; ++k) {
    const int c = cb[k * RB + rbl];
    const V* __restrict__ vk = vb + (int64_t)k * (BS * WAVE);
    const double* __restrict__ xb = x + (int64_t)c * (BS * NV);
    double xv[BS][NV];
#pragma unroll
    for (int cc = 0; cc < BS; ++cc) ldv<NV>(xb + cc * NV, xv[cc]);
#pragma unroll
    for (int cp = 0; cp < BS / 2; ++cp) {
      V v0, v1;
      ld_nt_pair(vk + cp * (2 * WAVE) + lane * 2, v0, v1);
#pragma unroll
      for (int j = 0; j < NV; ++j) {
        // (r = rest x on the float image, DESIGN.md 5.22: the pair sum spelled out, see bsell_block_step_nv)
        if constexpr (sizeof(V) == 4 && EP == EP_MULT) acc[j] += __builtin_fma((double)v0, xv[2 * cp][j], (double)v1 * xv[2 * cp + 1][j]);
        else acc[j] += (double)v0 * xv[2 * cp][j] + (double)v1 * xv[2 * cp + 1][j];
      }
    }
    if constexpr (BS & 1) {
      const double vl = (double)ld_nt(vk + (BS / 2) * (2 * WAVE) + lane);
#pragma unroll
      for (int j = 0; j < NV; ++j) acc[j] += vl * xv[BS - 1][j];
    }
  }
  block_row_epilogue_nv<BS, NV, EP>(active, brow, r, lane - r, acc, y, ep);
}

// Block CSR (BR x BC blocks), NV interleaved vectors: W lanes groups per block row, lane (g, r) owns scalar row r and the blocks
// g, g + W, ... of its block row (the lane layout of bcsr_rowlane_kernel).  ONE kernel for the small, latency-bound block levels and
// the transfers that are not rigid-body -- the single-vector path chooses between a row-per-lane and a block-per-lane kernel there.
// EP_JAC / EP_CHEB: square blocks only.
template <int BR, int BC, int NV, int EP, int W = 4>
__global__ __launch_bounds__(BLOCK) void bcsr_spmm_kernel(int64_t n_rows, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ cols,
                                                          const double* __restrict__ vals, const double* __restrict__ x, double* y, EpArgs ep) {
  constexpr int LPR = BR * W;                // lanes per block row
  constexpr int RPW = WAVE / LPR;            // block rows per wave
  const int lane = threadIdx.x & (WAVE - 1);
  const int64_t wave = (int64_t)blockIdx.x * WAVES_PER_BLOCK + (threadIdx.x >> 6);
  const int rloc = lane / LPR;
  const int g = (lane % LPR) / BR;
  const int r = lane % BR;
  const int64_t row = wave * RPW + rloc;
  const bool active = rloc < RPW && row < n_rows;
  double acc[NV];
#pragma unroll
  for (int j = 0; j < NV; ++j) acc[j] = 0.0;
  if (active) {
    const int e = rowptr[row + 1];
    for (int k = rowptr[row] + g; k < e; k += W) {
      const double* __restrict__ a = vals + (int64_t)k * (BR * BC) + r * BC;
      const double* __restrict__ xb = x + (int64_t)cols[k] * (BC * NV);
      double av[BC], xv[BC][NV];
#pragma unroll
      for (int c = 0; c < BC; ++c) av[c] = a[c];
#pragma unroll
      for (int c = 0; c < BC; ++c) ldv<NV>(xb + c * NV, xv[c]);
#pragma unroll
      for (int c = 0; c < BC; ++c) {
#pragma unroll
        for (int j = 0; j < NV; ++j) acc[j] += av[c] * xv[c][j];
      }
    }
  }
#pragma unroll
  for (int j = 0; j < NV; ++j) {
#pragma unroll
    for (int o = W >> 1; o > 0; o >>= 1) acc[j] += __shfl_down(acc[j], o * BR, WAVE);
  }
  // lanes with g == 0 now hold (A x)_r of their block row
  block_row_epilogue_nv<BR, NV, EP>(active && g == 0, row, r, lane - r, acc, y, ep);
}

// rigid-body transfer blocks on NV interleaved vectors: rb_forward / rb_transposed per column on (col, w, t) loaded once
template <int BF, int BC, int DIM, int NV, int EP>
__global__ __launch_bounds__(BLOCK) void rb_prolong_nv_kernel(int64_t n_rows, RbMat M, const double* __restrict__ x, double* y, EpArgs ep) {
  const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n_rows) return;
  double acc[NV][BF];
#pragma unroll
  for (int j = 0; j < NV; ++j)
#pragma unroll
    for (int r = 0; r < BF; ++r) acc[j][r] = 0.0;
  const int e = M.ptr[i + 1];
  for (int k = M.ptr[i]; k < e; ++k) {
    const double* __restrict__ xb = x + (int64_t)M.col[k] * (BC * NV);
    const double w = M.w[k];
    const double t0 = DIM >= 2 ? M.t[k] : 0.0, t1 = DIM >= 2 ? M.t[M.nnz + k] : 0.0, t2 = DIM == 3 ? M.t[2 * M.nnz + k] : 0.0;
    double xv[BC][NV];
#pragma unroll
    for (int c = 0; c < BC; ++c) ldv<NV>(xb + c * NV, xv[c]);
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      double xc[BC];
#pragma unroll
      for (int c = 0; c < BC; ++c) xc[c] = xv[c][j];
      rb_forward<BF, BC, DIM>(xc, w, t0, t1, t2, acc[j]);
    }
  }
#pragma unroll
  for (int r = 0; r < BF; ++r) {
    const int64_t io = (i * BF + r) * NV;
    double out[NV];
    if constexpr (EP == EP_AXPY) {
      double yin[NV];
      ldv<NV>(ep.yin + io, yin);
#pragma unroll
      for (int j = 0; j < NV; ++j) out[j] = yin[j] + ep.s * acc[j][r];
    } else {
      static_assert(EP == EP_MULT, "rigid-body transfer blocks: y = M x and y = yin + s M x only");
#pragma unroll
      for (int j = 0; j < NV; ++j) out[j] = acc[j][r];
    }
    stv<NV>(y + io, out);
  }
}
template <int BF, int BC, int DIM, int G, int NV, int EP>
__global__ __launch_bounds__(BLOCK) void rb_restrict_nv_kernel(int64_t n_rows, RbMat M, const double* __restrict__ x, double* y, EpArgs ep) {
  const int64_t tg = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  const int64_t J = tg / G;
  const int sub = (int)(tg % G);
  double acc[NV][BC];
#pragma unroll
  for (int j = 0; j < NV; ++j)
#pragma unroll
    for (int r = 0; r < BC; ++r) acc[j][r] = 0.0;
  if (J < n_rows) {
    const int e = M.ptr[J + 1];
    for (int k = M.ptr[J] + sub; k < e; k += G) {
      const double* __restrict__ xb = x + (int64_t)M.col[k] * (BF * NV);
      const double w = M.w[k];
      const double t0 = DIM >= 2 ? M.t[k] : 0.0, t1 = DIM >= 2 ? M.t[M.nnz + k] : 0.0, t2 = DIM == 3 ? M.t[2 * M.nnz + k] : 0.0;
      double xv[BF][NV];
#pragma unroll
      for (int c = 0; c < BF; ++c) ldv<NV>(xb + c * NV, xv[c]);
#pragma unroll
      for (int j = 0; j < NV; ++j) {
        double rf[BF];
#pragma unroll
        for (int c = 0; c < BF; ++c) rf[c] = xv[c][j];
        rb_transposed<BF, BC, DIM>(rf, w, t0, t1, t2, acc[j]);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < NV; ++j)
#pragma unroll
    for (int r = 0; r < BC; ++r)
#pragma unroll
      for (int o = G >> 1; o > 0; o >>= 1) acc[j][r] += __shfl_xor(acc[j][r], o, G);
  if (J < n_rows && sub == 0) {
#pragma unroll
    for (int r = 0; r < BC; ++r) {
      const int64_t io = (J * BC + r) * NV;
      double out[NV];
      if constexpr (EP == EP_AXPY) {
        double yin[NV];
        ldv<NV>(ep.yin + io, yin);
#pragma unroll
        for (int j = 0; j < NV; ++j) out[j] = yin[j] + ep.s * acc[j][r];
      } else {
        static_assert(EP == EP_MULT, "rigid-body transfer blocks: y = M x and y = yin + s M x only");
#pragma unroll
        for (int j = 0; j < NV; ++j) out[j] = acc[j][r];
      }
      stv<NV>(y + io, out);
    }
  }
}

// dense Y = M X for NV interleaved vectors, one wave per row: the coarse inverse and the collapsed dense operator are read once
template <int NV>
__global__ __launch_bounds__(BLOCK) void dense_gemm_nv_kernel(int n, int ld, const double* __restrict__ M, const double* __restrict__ x, double* __restrict__ y) {
  const int row = blockIdx.x * WAVES_PER_BLOCK + (threadIdx.x >> 6);
  const int lane = threadIdx.x & (WAVE - 1);
  if (row >= n) return;
  const double* __restrict__ m = M + (int64_t)row * ld;
  double acc[NV];
#pragma unroll
  for (int j = 0; j < NV; ++j) acc[j] = 0.0;
  int c = lane;
  for (; c + 3 * WAVE < n; c += 4 * WAVE) {     // four matrix loads and their gathers in flight per lane
    double mv[4], xv[4][NV];
#pragma unroll
    for (int q = 0; q < 4; ++q) mv[q] = m[c + q * WAVE];
#pragma unroll
    for (int q = 0; q < 4; ++q) ldv<NV>(x + (int64_t)(c + q * WAVE) * NV, xv[q]);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
#pragma unroll
      for (int j = 0; j < NV; ++j) acc[j] += mv[q] * xv[q][j];
    }
  }
  for (; c < n; c += WAVE) {
    const double mv = m[c];
    double xv[NV];
    ldv<NV>(x + (int64_t)c * NV, xv);
#pragma unroll
    for (int j = 0; j < NV; ++j) acc[j] += mv * xv[j];
  }
#pragma unroll
  for (int j = 0; j < NV; ++j) {
#pragma unroll
    for (int o = WAVE >> 1; o > 0; o >>= 1) acc[j] += __shfl_xor(acc[j], o, WAVE);
  }
  if (lane == 0) stv<NV>(y + (int64_t)row * NV, acc);
}

// ---- Gauss-Seidel sweeps on NV interleaved vectors (AMGX_MULTI_FUSE_GS) ----------------------------------------
// gsb_sweep_kernel (kernels.hpp) for NV vectors: the same image, the same slot -> row map, the same colour phases and barriers; the
// matrix values and the decoded columns of a lane are loaded ONCE and serve all NV columns.  Per column the arithmetic is that of
// the single-vector kernel -- acc_off over the lane's entries j ascending, the __shfl_xor tree over the G lanes of a row, colours in
// the same order, x_k + dinv_k * (b_k - acc_off - acc) -- and no operation mixes two columns.
//   * the block's x lives in LDS interleaved like the vectors (B * NV doubles: 32 KB at B = 1024, NV = 4); b and dinv of a row are
//     read by the row's writer lane straight from memory (NV contiguous doubles), so the LDS need stays below the 64 KB a launch can
//     have for every (B, NV) and the plan has nothing to refuse;
//   * the off-block gathers are consumed in batches of GB entries (GB * NV doubles in flight per lane): all 2 * WP + 1 at once would
//     be 17 * NV doubles, beyond the register budget of a 1024-lane workgroup;
//   * plain images only (global columns): the local-window and mid-width forms of the single-vector sweep are launch choices over
//     the same slot order, so their results are the same bits.
// The colour loop holds a workgroup barrier: no lane returns before it, n_colors is uniform.
// V = float (AMGX_MULTI_FUSE_F32): the single-precision image, same index arrays; a lane keeps its values as loaded
// and widens them where it multiplies, as gsb_sweep_kernel<..., float> does.
template <int TH, int G, bool FROM_ZERO, int WP, int NV, class V = double>
__global__ __launch_bounds__(TH) void gsb_sweep_nv_kernel(int64_t n_rows, SellMatT<V> M, GsbArgs a, const double* __restrict__ xin, double* xout) {
  constexpr int B = TH / G;                  // rows per block
  constexpr int RPS = WAVE / G;              // rows per slice
  constexpr int NE = 2 * WP + 1;             // entries a lane holds
  constexpr int XQ = (B * NV + TH - 1) / TH; // entries of the block's x per thread
  constexpr int GB = NV <= 2 ? 4 : 2;        // off-block entries gathered per batch
  __shared__ __attribute__((aligned(16))) double xs[B * NV];
  const int blk = blockIdx.x;
  const int64_t r0 = (int64_t)blk * B;
  const int tid = threadIdx.x, lane = tid & (WAVE - 1);
  const int s = __builtin_amdgcn_readfirstlane(blk * (TH / WAVE) + (tid >> 6));
  // ---- phase 1: every load that depends on nothing
  const int64_t x0 = r0 * NV;
  const int64_t xend = (n_rows - r0 < B ? n_rows - r0 : (int64_t)B) * NV;       // entries of the block that exist (last block: partial)
  double x_own[XQ];
#pragma unroll
  for (int q = 0; q < XQ; ++q) {
    const int k = tid + q * TH;
    x_own[q] = 0.0;
    if (!FROM_ZERO) { if (k < xend) x_own[q] = xin[x0 + k]; }
  }
  const int slot = s * RPS + lane / G;
  const int row = a.rowid[slot];
  const int col_raw = (int)a.slotcolor[slot];
  const int64_t sp0 = M.slice_ptr[s];
  const int64_t base = sp0 & ~(int64_t)63;
  const int w = (int)(((M.slice_ptr[s + 1] & ~(int64_t)63) - base) >> 6);
  const int np = w >> 1;
  const bool c16 = sp0 & 1;
  const V* __restrict__ vb = M.val + base;
  const int32_t* __restrict__ cb = M.cbase + (base >> 6);
  V v[NE];
  int cl[NE];
  uint32_t ra[WP], rb[WP];
#pragma unroll
  for (int p = 0; p < WP; ++p) {
    v[2 * p] = 0; v[2 * p + 1] = 0; ra[p] = 0; rb[p] = 0;
    if (p < np) {                                            // wave-uniform
      ld_nt_pair(vb + (p * WAVE + lane) * 2, v[2 * p], v[2 * p + 1]);
      if (c16) ra[p] = ld_nt(reinterpret_cast<const uint32_t*>(M.col16 + base) + p * WAVE + lane);
      else {
        ra[p] = (uint32_t)ld_nt(M.col32 + base + (p * WAVE + lane) * 2);
        rb[p] = (uint32_t)ld_nt(M.col32 + base + (p * WAVE + lane) * 2 + 1);
      }
    }
  }
  int cbv[NE];                           // column bases of the slice (the array has slack at its end, see gsb_sweep_kernel)
#pragma unroll
  for (int j = 0; j < NE; ++j) cbv[j] = 0;
  if (c16) {
#pragma unroll
    for (int j = 0; j < NE; ++j) cbv[j] = cb[j];
  }
  uint32_t rt = 0;
  v[2 * WP] = 0;
  if (w & 1) {
    const int64_t o = (int64_t)(w - 1) * WAVE + lane;
    v[2 * WP] = ld_nt(vb + o);
    rt = c16 ? (uint32_t)ld_nt(M.col16 + base + o) : (uint32_t)ld_nt(M.col32 + base + o);
  }
  // own-row operands of the writer lanes: NV contiguous doubles of b, one dinv
  const int mycol = row >= 0 ? col_raw : 255;
  const bool writer = mycol != 255 && (lane % G) == 0;
  double bv[NV], dv = 0.0;
#pragma unroll
  for (int c = 0; c < NV; ++c) bv[c] = 0.0;
  if (writer) { ldv<NV>(a.b + (int64_t)row * NV, bv); dv = a.dinv[row]; }
  // ---- phase 2: the column decode
#pragma unroll
  for (int p = 0; p < WP; ++p) {
    cl[2 * p] = (int)r0; cl[2 * p + 1] = (int)r0;
    if (p < np) {
      if (c16) { cl[2 * p] = cbv[2 * p] + (int)(ra[p] & 0xffffu); cl[2 * p + 1] = cbv[2 * p + 1] + (int)(ra[p] >> 16); }
      else { cl[2 * p] = (int)ra[p]; cl[2 * p + 1] = (int)rb[p]; }
    }
  }
  int cbt = 0;
#pragma unroll
  for (int j = 0; j < NE; j += 2) cbt = (w - 1 == j) ? cbv[j] : cbt;
  cl[2 * WP] = (w & 1) ? (c16 ? cbt + (int)rt : (int)rt) : (int)r0;
  // the block's x goes to LDS here: its loads were the first ones requested, and their registers are free before the gathers start
#pragma unroll
  for (int q = 0; q < XQ; ++q) {
    const int k = tid + q * TH;
    if (k < B * NV) xs[k] = x_own[q];
  }
  // ---- phase 3: off-block part (sweep-start values), GB entries per batch; in-block entries keep (value, LDS slot).  The empty
  // asm after a batch pins the batch's sums before the next batch's loads: without it the compiler requests the gathers of all
  // batches at once and keeps every product (222-232 VGPRs at NV = 4, spills in the 1024-lane workgroups)
  double acc_off[NV];
#pragma unroll
  for (int c = 0; c < NV; ++c) acc_off[c] = 0.0;
#pragma unroll
  for (int j0 = 0; j0 < NE; j0 += GB) {
    double xg[GB][NV];
    bool inb[GB];
#pragma unroll
    for (int u = 0; u < GB; ++u) {
      if (j0 + u < NE) {
        const int j = j0 + u;
        const int loc = cl[j] - (int)r0;
        inb[u] = loc >= 0 && loc < B && cl[j] < n_rows;
#pragma unroll
        for (int c = 0; c < NV; ++c) xg[u][c] = 0.0;
        // (an in-block entry reads the block's first row instead and drops the value: straight-line code, no branch per entry)
        if (!FROM_ZERO) ldv<NV>(xin + (inb[u] ? x0 : (int64_t)cl[j] * NV), xg[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < GB; ++u) {
      if (j0 + u < NE) {
        const int j = j0 + u;
        if (!FROM_ZERO) {
#pragma unroll
          for (int c = 0; c < NV; ++c) acc_off[c] += inb[u] ? 0.0 : (double)v[j] * xg[u][c];
        }
        if (inb[u]) cl[j] -= (int)r0;
        else { v[j] = 0; cl[j] = 0; }
      }
    }
    if (!FROM_ZERO) {
#pragma unroll
      for (int c = 0; c < NV; ++c) asm volatile("" : "+v"(acc_off[c]) : : "memory");
    }
  }
#pragma unroll
  for (int c = 0; c < NV; ++c) {
#pragma unroll
    for (int o = G >> 1; o > 0; o >>= 1) acc_off[c] += __shfl_xor(acc_off[c], o, G);
  }
  const int own = row >= 0 ? row - (int)r0 : 0;
  __syncthreads();                                           // xs is loaded
  for (int q = 0; q < a.n_colors; ++q) {
    const int c = a.backward ? a.n_colors - 1 - q : q;
    if (__any(mycol == c)) {
      double acc[NV];
#pragma unroll
      for (int cc = 0; cc < NV; ++cc) acc[cc] = 0.0;
#pragma unroll
      for (int j = 0; j < NE; ++j) {
        double xv[NV];
        ldv<NV>(xs + cl[j] * NV, xv);
#pragma unroll
        for (int cc = 0; cc < NV; ++cc) acc[cc] += (double)v[j] * xv[cc];
      }
#pragma unroll
      for (int cc = 0; cc < NV; ++cc) {
#pragma unroll
        for (int o = G >> 1; o > 0; o >>= 1) acc[cc] += __shfl_xor(acc[cc], o, G);
      }
      if (writer && mycol == c) {
        double xo[NV];
        ldv<NV>(xs + own * NV, xo);
#pragma unroll
        for (int cc = 0; cc < NV; ++cc) xo[cc] = xo[cc] + dv * (bv[cc] - acc_off[cc] - acc[cc]);
        stv<NV>(xs + own * NV, xo);
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int q = 0; q < XQ; ++q) {
    const int k = tid + q * TH;
    if (k < xend) xout[x0 + k] = xs[k];
  }
}

// gs_color_kernel (kernels.hpp) with the row product widened to NV gathers: one colour per launch on the colour-major images `sell`
// and `lower` of DevGS.  Padding rows (rowid < 0) are never written.
template <int G, int NV, class V = double>
__global__ __launch_bounds__(BLOCK) void gs_color_nv_kernel(int slice_begin, int slice_end, SellMatT<V> M, const int32_t* __restrict__ rowid,
                                                            const double* __restrict__ dinv, const double* __restrict__ b, double* x) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int s = __builtin_amdgcn_readfirstlane(slice_begin + blockIdx.x * WAVES_PER_BLOCK + (threadIdx.x >> 6));
  if (s >= slice_end) return;
  const int row = rowid[(int64_t)s * (WAVE / G) + lane / G];
  const bool writer = row >= 0 && (lane % G) == 0;
  double dv = 0.0, bv[NV], xv[NV], acc[NV];
#pragma unroll
  for (int j = 0; j < NV; ++j) { bv[j] = 0.0; xv[j] = 0.0; acc[j] = 0.0; }
  if (writer) { dv = dinv[row]; ldv<NV>(b + (int64_t)row * NV, bv); ldv<NV>(x + (int64_t)row * NV, xv); }
  if (row >= 0) sell_row_dot_nv<NV>(M, s, lane, row, x, acc);
#pragma unroll
  for (int j = 0; j < NV; ++j) {
#pragma unroll
    for (int o = G >> 1; o > 0; o >>= 1) acc[j] += __shfl_xor(acc[j], o, G);
  }
  if (writer) {
#pragma unroll
    for (int j = 0; j < NV; ++j) xv[j] = xv[j] + dv * (bv[j] - acc[j]);
    stv<NV>(x + (int64_t)row * NV, xv);
  }
}

// gs_upper_residual_kernel for NV vectors: r = -(U x) on the colour-major rows of the `upper` image, right after a forward sweep
// from x = 0
template <int G, int NV, class V = double>
__global__ __launch_bounds__(BLOCK) void gs_upper_residual_nv_kernel(int n_slices, SellMatT<V> M, const int32_t* __restrict__ rowid,
                                                                     const double* __restrict__ x, double* __restrict__ r) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int s = __builtin_amdgcn_readfirstlane(blockIdx.x * WAVES_PER_BLOCK + (threadIdx.x >> 6));
  if (s >= n_slices) return;
  const int row = rowid[(int64_t)s * (WAVE / G) + lane / G];
  double acc[NV];
#pragma unroll
  for (int j = 0; j < NV; ++j) acc[j] = 0.0;
  if (row >= 0) sell_row_dot_nv<NV>(M, s, lane, row, x, acc);
#pragma unroll
  for (int j = 0; j < NV; ++j) {
#pragma unroll
    for (int o = G >> 1; o > 0; o >>= 1) acc[j] += __shfl_xor(acc[j], o, G);
  }
  if (row >= 0 && (lane % G) == 0) {
#pragma unroll
    for (int j = 0; j < NV; ++j) acc[j] = -acc[j];
    stv<NV>(r + (int64_t)row * NV, acc);
  }
}

// ---- Gauss-Seidel sweeps of SQUARE-BLOCK levels on NV interleaved vectors (AMGX_MULTI_FUSE_GS_BLOCK) -----------
// One block step of a BSELL row product for NV columns: the value loads of bsell_block_step<BS, false> (pair order, odd trailing
// column last) and ONE gather of the block's BS * NV contiguous doubles at xb (global memory or LDS).  The values are loaded once
// and serve all NV columns; per column the additions are those of the single-vector step.
// V = float: the single-precision image; a value is widened where it multiplies (bsell_block_step<BS, false, float>).
template <int BS, int NV, class V>
__device__ __forceinline__ void bsell_block_step_nv(const V* __restrict__ vk, const double* xb, int lane, double (&acc)[NV]) {
  double xv[BS][NV];
#pragma unroll
  for (int cc = 0; cc < BS; ++cc) ldv<NV>(xb + cc * NV, xv[cc]);
#pragma unroll
  for (int cp = 0; cp < BS / 2; ++cp) {
    V v0, v1;
    ld_nt_pair(vk + cp * (2 * WAVE) + lane * 2, v0, v1);
    // (float: the pair sum is written as the fused multiply-add every other kernel of the family compiles to, v0 x0 + [v1 x1]; left to
    // the compiler, the widened operands come out as [v0 x0] + v1 x1 in some columns -- another rounding, measured 7e-15 per sweep)
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      if constexpr (sizeof(V) == 4) acc[j] += __builtin_fma((double)v0, xv[2 * cp][j], (double)v1 * xv[2 * cp + 1][j]);
      else acc[j] += v0 * xv[2 * cp][j] + v1 * xv[2 * cp + 1][j];
    }
  }
  if constexpr (BS & 1) {
    const double vl = (double)ld_nt(vk + (BS / 2) * (2 * WAVE) + lane);
#pragma unroll
    for (int j = 0; j < NV; ++j) acc[j] += vl * xv[BS - 1][j];
  }
}
// (row product of one slice: `w` block steps from (vb, cb), gathered blocks at x + c * BS * NV)
template <int BS, int NV, class V>
__device__ __forceinline__ void bsell_slice_dot_nv(const BSellMatT<V>& M, int s, int rbl, int lane, const double* x, double (&acc)[NV]) {
  constexpr int RB = WAVE / BS;
  const int64_t k0 = M.slice_ptr[s];
  const int w = (int)(M.slice_ptr[s + 1] - k0);
  const V* __restrict__ vb = M.val + k0 * (BS * WAVE);
  const int32_t* __restrict__ cb = M.col + k0 * RB;
#pragma unroll
  for (int j = 0; j < NV; ++j) acc[j] = 0.0;
  for (int k = 0; k < w; ++k) {
    const int c = cb[k * RB + rbl];
    bsell_block_step_nv<BS, NV, V>(vb + (int64_t)k * (BS * WAVE), x + (int64_t)c * (BS * NV), lane, acc);
  }
}
// the block solve of a row's lane group for NV columns: u = sum_c od[c] * t_c with t exchanged over the BS lanes from `base` on
// (the __shfl order of the single-vector kernels).  Every lane of the wave calls it.
template <int BS, int NV>
__device__ __forceinline__ void block_solve_nv(const double (&od)[BS], const double (&t)[NV], int base, double (&u)[NV]) {
#pragma unroll
  for (int j = 0; j < NV; ++j) u[j] = 0.0;
#pragma unroll
  for (int cc = 0; cc < BS; ++cc) {
#pragma unroll
    for (int j = 0; j < NV; ++j) u[j] += od[cc] * __shfl(t[j], base + cc, WAVE);
  }
}

// bgsb_sweep_kernel (kernels.hpp) for NV vectors: the same images (off / offlo, in, upin), the same blk_ptr / blk_rows / blk_list /
// off_ptr / in_ptr / in_row, the same phases, colours and barriers; MODE as there (0: general, 1: from zero, 2: block-coloured from
// zero, later block colours).  xs and b' live in LDS interleaved like the vectors (2 * BB * BS * NV doubles + the BB row ids: the
// launcher computes the size, Handle::multi_block_sweep_lds); a row's dinv is loaded once for all NV columns.  Every lane reaches
// every barrier; idle lanes (lane >= RB * BS) and padding slots (in_row < 0) never write.
template <int BS, int MODE, int NV, class V = double>
__global__ __launch_bounds__(BLOCK) void bgsb_sweep_nv_kernel(int BB, int block0, const int32_t* __restrict__ blk_list,
                                                              const int32_t* __restrict__ blk_ptr, const int32_t* __restrict__ blk_rows,
                                                              BSellMatT<V> OFF, const int32_t* __restrict__ off_ptr,
                                                              BSellMatT<V> IN, BSellMatT<V> OTH, const int32_t* __restrict__ in_ptr, const int32_t* __restrict__ in_row,
                                                              int n_colors, int dir, const double* __restrict__ dinv, const double* __restrict__ b,
                                                              const double* xin, double* xout) {
  constexpr bool FROM_ZERO = MODE != 0;
  constexpr int RB = WAVE / BS;
  constexpr int RW = BS * NV;                // doubles of one block row
  extern __shared__ __attribute__((aligned(16))) double bgsb_nv_sh[];
  double* xs = bgsb_nv_sh;
  double* bsh = bgsb_nv_sh + (size_t)BB * RW;
  int* rowsh = reinterpret_cast<int*>(bgsb_nv_sh + (size_t)2 * BB * RW);     // global block row of every local row
  const int blk = blk_list ? blk_list[block0 + blockIdx.x] : block0 + blockIdx.x;
  const int p0 = blk_ptr[blk];
  const int nb = blk_ptr[blk + 1] - p0;
  for (int e = threadIdx.x; e < nb; e += BLOCK) rowsh[e] = blk_rows[p0 + e];
  __syncthreads();
  for (int e = threadIdx.x; e < nb * RW; e += BLOCK) {
    const int64_t g = (int64_t)rowsh[e / RW] * RW + e % RW;
    xs[e] = FROM_ZERO ? 0.0 : xin[g];
    bsh[e] = b[g];
  }
  __syncthreads();
  const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x >> 6;
  const int rbl = lane / BS < RB ? lane / BS : RB - 1;
  const int r = lane % BS;
  const bool lane_on = lane < RB * BS;
  if (MODE != 1) {
    // phase 0: b' = b - (A_off + A_oth) x_old, gathers from global memory / from LDS
    const int s0 = off_ptr[blk], s1 = off_ptr[blk + 1];
    for (int s = s0 + wave; s < s1; s += WAVES_PER_BLOCK) {
      const int lrow = (s - s0) * RB + rbl;
      const bool active = lane_on && lrow < nb;
      double acc[NV];
      bsell_slice_dot_nv<BS, NV, V>(OFF, s, rbl, lane, xin, acc);
      if (active) {
        double bb[NV];
        ldv<NV>(bsh + (lrow * BS + r) * NV, bb);
#pragma unroll
        for (int j = 0; j < NV; ++j) bb[j] -= acc[j];
        stv<NV>(bsh + (lrow * BS + r) * NV, bb);
      }
    }
    __syncthreads();
    const int t0 = in_ptr[blk * n_colors], t1 = MODE == 0 ? in_ptr[(blk + 1) * n_colors] : t0;
    for (int s = t0 + wave; s < t1; s += WAVES_PER_BLOCK) {
      const int lrow = in_row[(int64_t)s * RB + rbl];
      const bool active = lane_on && lrow >= 0;
      double acc[NV];
      bsell_slice_dot_nv<BS, NV, V>(OTH, s, rbl, lane, xs, acc);
      if (active) {
        double bb[NV];
        ldv<NV>(bsh + (lrow * BS + r) * NV, bb);
#pragma unroll
        for (int j = 0; j < NV; ++j) bb[j] -= acc[j];
        stv<NV>(bsh + (lrow * BS + r) * NV, bb);
      }
    }
    __syncthreads();
  }
  for (int q = 0; q < n_colors; ++q) {
    const int c = dir ? n_colors - 1 - q : q;
    const int s0 = in_ptr[blk * n_colors + c], s1 = in_ptr[blk * n_colors + c + 1];
    for (int s = s0 + wave; s < s1; s += WAVES_PER_BLOCK) {
      const int lrow = in_row[(int64_t)s * RB + rbl];
      const bool active = lane_on && lrow >= 0;
      double od[BS];
#pragma unroll
      for (int cc = 0; cc < BS; ++cc) od[cc] = active ? dinv[(int64_t)rowsh[lrow] * (BS * BS) + r * BS + cc] : 0.0;
      double acc[NV], t[NV], u[NV];
      bsell_slice_dot_nv<BS, NV, V>(IN, s, rbl, lane, xs, acc);
#pragma unroll
      for (int j = 0; j < NV; ++j) t[j] = 0.0;
      if (active) {
        ldv<NV>(bsh + (lrow * BS + r) * NV, t);
#pragma unroll
        for (int j = 0; j < NV; ++j) t[j] = t[j] - acc[j];
      }
      block_solve_nv<BS, NV>(od, t, lane - r, u);
      if (active) {
        double xo[NV];
        ldv<NV>(xs + (lrow * BS + r) * NV, xo);
#pragma unroll
        for (int j = 0; j < NV; ++j) xo[j] += u[j];
        stv<NV>(xs + (lrow * BS + r) * NV, xo);
      }
    }
    __syncthreads();
  }
  for (int e = threadIdx.x; e < nb * RW; e += BLOCK) xout[(int64_t)rowsh[e / RW] * RW + e % RW] = xs[e];
}

// bgs_bsell_color_kernel for NV vectors: one colour per launch on the colour-major BSELL copy (gs.bcopy, or gs.blower for the sweep
// from zero), in place.  Padding slots (rowid < 0) and idle lanes never write.
template <int BS, int NV, class V = double>
__global__ __launch_bounds__(BLOCK) void bgs_bsell_color_nv_kernel(int slice_begin, int slice_end, BSellMatT<V> M, const int32_t* __restrict__ rowid,
                                                                   const double* __restrict__ dinv, const double* __restrict__ b, double* x) {
  constexpr int RB = WAVE / BS;
  const int lane = threadIdx.x & (WAVE - 1);
  const int s = __builtin_amdgcn_readfirstlane(slice_begin + blockIdx.x * WAVES_PER_BLOCK + (threadIdx.x >> 6));
  if (s >= slice_end) return;
  const int rbl = lane / BS < RB ? lane / BS : RB - 1;
  const int r = lane % BS;
  const int brow = rowid[(int64_t)s * RB + rbl];
  const bool active = lane < RB * BS && brow >= 0;
  const int64_t io = ((int64_t)(brow >= 0 ? brow : 0) * BS + r) * NV;
  double t[NV], od[BS];
#pragma unroll
  for (int j = 0; j < NV; ++j) t[j] = 0.0;
#pragma unroll
  for (int c = 0; c < BS; ++c) od[c] = 0.0;
  if (active) {
    ldv<NV>(b + io, t);
#pragma unroll
    for (int c = 0; c < BS; ++c) od[c] = dinv[(int64_t)brow * (BS * BS) + r * BS + c];
  }
  double acc[NV], u[NV];
  bsell_slice_dot_nv<BS, NV, V>(M, s, rbl, lane, x, acc);
#pragma unroll
  for (int j = 0; j < NV; ++j) t[j] = active ? t[j] - acc[j] : 0.0;
  block_solve_nv<BS, NV>(od, t, lane - r, u);
  if (active) {
    double xo[NV];
    ldv<NV>(x + io, xo);
#pragma unroll
    for (int j = 0; j < NV; ++j) xo[j] += u[j];
    stv<NV>(x + io, xo);
  }
}

// bgs_bsell_upper_residual_kernel for NV vectors: r_B = -(U x)_B on the colour-major block rows of gs.bupper after the sweep from zero
template <int BS, int NV, class V = double>
__global__ __launch_bounds__(BLOCK) void bgs_bsell_upper_residual_nv_kernel(int n_slices, BSellMatT<V> M, const int32_t* __restrict__ rowid,
                                                                            const double* __restrict__ x, double* __restrict__ res) {
  constexpr int RB = WAVE / BS;
  const int lane = threadIdx.x & (WAVE - 1);
  const int s = __builtin_amdgcn_readfirstlane(blockIdx.x * WAVES_PER_BLOCK + (threadIdx.x >> 6));
  if (s >= n_slices) return;
  const int rbl = lane / BS < RB ? lane / BS : RB - 1;
  const int r = lane % BS;
  const int brow = rowid[(int64_t)s * RB + rbl];
  const bool active = lane < RB * BS && brow >= 0;
  double acc[NV];
  bsell_slice_dot_nv<BS, NV, V>(M, s, rbl, lane, x, acc);
  if (active) {
#pragma unroll
    for (int j = 0; j < NV; ++j) acc[j] = -acc[j];
    stv<NV>(res + ((int64_t)brow * BS + r) * NV, acc);
  }
}

// bgs_color_kernel for NV vectors: the colour-major row list over the block CSR of A, lane (g, r) owns scalar row r and the blocks
// g, g + W, ... of its block row (the additions of bcsr_row_dot per column: blocks ascending, block columns ascending)
template <int BS, int W, int NV>
__global__ __launch_bounds__(BLOCK) void bgs_color_nv_kernel(int list_begin, int list_end, const int32_t* __restrict__ rowlist,
                                                             const int32_t* __restrict__ rowptr, const int32_t* __restrict__ cols,
                                                             const double* __restrict__ vals, const double* __restrict__ dinv,
                                                             const double* __restrict__ b, double* x) {
  constexpr int LPR = BS * W;
  constexpr int RPW = WAVE / LPR;
  const int lane = threadIdx.x & (WAVE - 1);
  const int64_t wave = (int64_t)blockIdx.x * WAVES_PER_BLOCK + (threadIdx.x >> 6);
  const int rloc = lane / LPR;
  const int g = (lane % LPR) / BS;
  const int r = lane % BS;
  const int64_t q = list_begin + wave * RPW + rloc;
  const bool active = rloc < RPW && q < list_end;
  const int row = active ? rowlist[q] : 0;
  double acc[NV];
#pragma unroll
  for (int j = 0; j < NV; ++j) acc[j] = 0.0;
  if (active) {
    const int e = rowptr[row + 1];
    for (int k = rowptr[row] + g; k < e; k += W) {
      const double* __restrict__ a = vals + (int64_t)k * (BS * BS) + r * BS;
      const double* xb = x + (int64_t)cols[k] * (BS * NV);
      double av[BS], xv[BS][NV];
#pragma unroll
      for (int c = 0; c < BS; ++c) av[c] = a[c];
#pragma unroll
      for (int c = 0; c < BS; ++c) ldv<NV>(xb + c * NV, xv[c]);
#pragma unroll
      for (int c = 0; c < BS; ++c) {
#pragma unroll
        for (int j = 0; j < NV; ++j) acc[j] += av[c] * xv[c][j];
      }
    }
  }
#pragma unroll
  for (int j = 0; j < NV; ++j) {
#pragma unroll
    for (int o = W >> 1; o > 0; o >>= 1) acc[j] += __shfl_down(acc[j], o * BS, WAVE);
  }
  const bool writer = active && g == 0;
  const int64_t io = ((int64_t)row * BS + r) * NV;
  double t[NV], od[BS], u[NV];
#pragma unroll
  for (int j = 0; j < NV; ++j) t[j] = 0.0;
#pragma unroll
  for (int c = 0; c < BS; ++c) od[c] = 0.0;
  if (writer) {
    ldv<NV>(b + io, t);
#pragma unroll
    for (int j = 0; j < NV; ++j) t[j] = t[j] - acc[j];
#pragma unroll
    for (int c = 0; c < BS; ++c) od[c] = dinv[(int64_t)row * (BS * BS) + r * BS + c];
  }
  block_solve_nv<BS, NV>(od, t, lane - r, u);
  if (writer) {
    double xo[NV];
    ldv<NV>(x + io, xo);
#pragma unroll
    for (int j = 0; j < NV; ++j) xo[j] += u[j];
    stv<NV>(x + io, xo);
  }
}

// ---- element-wise pieces on interleaved vectors (one thread per entry) -------------------------------------------------------
// x = omega * Dinv * b, width 1 << sh     (diag_apply_kernel<1, false> per column)
__global__ __launch_bounds__(BLOCK) void multi_diag_kernel(int64_t len, int sh, const double* __restrict__ dinv, const double* __restrict__ b,
                                                           double* __restrict__ x, double omega) {
  const int64_t t = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (t < len) x[t] = omega * (dinv[t >> sh] * b[t]);
}
// block form: x = c * Dinv_block * b per column, one thread per (block row, column); width nv.  The Jacobi first step with c = omega
// (diag_apply_kernel per column) and the Chebyshev first step from zero with c = c0 (cheb_first_kernel per column)
template <int BS>
__global__ __launch_bounds__(BLOCK) void multi_bdiag_kernel(int64_t n_blocks, int nv, const double* __restrict__ dinv, const double* __restrict__ b,
                                                            double* __restrict__ x, double c0) {
  const int64_t t = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (t >= n_blocks * nv) return;
  const int64_t i = t / nv;
  const int j = (int)(t - i * nv);
  double vv[BS];
#pragma unroll
  for (int c = 0; c < BS; ++c) vv[c] = b[(i * BS + c) * nv + j];
  const double* __restrict__ d = dinv + i * (BS * BS);
#pragma unroll
  for (int r = 0; r < BS; ++r) {
    double u = 0.0;
#pragma unroll
    for (int c = 0; c < BS; ++c) u += d[r * BS + c] * vv[c];
    u *= c0;
    x[(i * BS + r) * nv + j] = u;
  }
}
// dst[i*w + j] = src[i*rs + (c0 + j)*cs]: columns c0 .. c0+w of a column-major (rs = 1, cs = ld) or interleaved (rs = k, cs = 1)
// multi-vector into an interleaved one of width w
__global__ __launch_bounds__(BLOCK) void multi_pack_kernel(int64_t n, int w, const double* __restrict__ src, int64_t rs, int64_t cs, int c0,
                                                           double* __restrict__ dst) {
  const int64_t t = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (t >= n * w) return;
  const int64_t i = t / w;
  const int j = (int)(t - i * w);
  dst[t] = src[i * rs + (c0 + j) * cs];
}
// and back
__global__ __launch_bounds__(BLOCK) void multi_unpack_kernel(int64_t n, int w, const double* __restrict__ src, double* __restrict__ dst, int64_t rs,
                                                             int64_t cs, int c0) {
  const int64_t t = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (t >= n * w) return;
  const int64_t i = t / w;
  const int j = (int)(t - i * w);
  dst[i * rs + (c0 + j) * cs] = src[t];
}

// ---- BLAS-1 of the k independent CG recurrences, interleaved vectors, one launch per operation for all columns ---------------
// partial[j * KR_BLOCKS + block] = this block's grid-stride share of <a_j, b_j>; kr_dot_final_kernel adds them (fixed order)
__global__ __launch_bounds__(BLOCK) void kr_dot_multi_partial_kernel(int64_t n, int k, const double* __restrict__ a, const double* __restrict__ b,
                                                                     double* __restrict__ partial) {
  __shared__ double red[MULTI_MAX][BLOCK / WAVE];
  double acc[MULTI_MAX];
#pragma unroll
  for (int j = 0; j < MULTI_MAX; ++j) acc[j] = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * BLOCK) {
#pragma unroll
    for (int j = 0; j < MULTI_MAX; ++j)
      if (j < k) acc[j] += a[i * k + j] * b[i * k + j];
  }
#pragma unroll
  for (int j = 0; j < MULTI_MAX; ++j) {
#pragma unroll
    for (int o = WAVE >> 1; o > 0; o >>= 1) acc[j] += __shfl_xor(acc[j], o, WAVE);
    if ((threadIdx.x & (WAVE - 1)) == 0) red[j][threadIdx.x >> 6] = acc[j];
  }
  __syncthreads();
  if ((int)threadIdx.x < k) {
    double s = 0.0;
    for (int w = 0; w < BLOCK / WAVE; ++w) s += red[threadIdx.x][w];
    partial[(int64_t)threadIdx.x * KR_BLOCKS + blockIdx.x] = s;
  }
}
// x_j += alpha_j s_j, d_j -= alpha_j q_j with alpha_j = num[j] / den[j]; columns with active[j] == 0 are not touched
__global__ __launch_bounds__(BLOCK) void kr_cg_update_multi_kernel(int64_t len, int k, const double* __restrict__ num, const double* __restrict__ den,
                                                                   const int32_t* __restrict__ active, const double* __restrict__ s,
                                                                   const double* __restrict__ q, double* __restrict__ x, double* __restrict__ d) {
  const int64_t t = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (t >= len) return;
  const int j = (int)(t % k);
  if (!active[j]) return;
  const double alpha = num[j] / den[j];
  x[t] += alpha * s[t];
  d[t] -= alpha * q[t];
}
// s_j = w_j + (num[j] / den[j]) s_j on the active columns
__global__ __launch_bounds__(BLOCK) void kr_xpby_multi_kernel(int64_t len, int k, const double* __restrict__ num, const double* __restrict__ den,
                                                              const int32_t* __restrict__ active, const double* __restrict__ w, double* __restrict__ s) {
  const int64_t t = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (t >= len) return;
  const int j = (int)(t % k);
  if (!active[j]) return;
  s[t] = w[t] + (num[j] / den[j]) * s[t];
}
// d = b - w
__global__ __launch_bounds__(BLOCK) void multi_sub_kernel(int64_t len, const double* __restrict__ b, const double* __restrict__ w, double* __restrict__ d) {
  const int64_t t = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (t < len) d[t] = b[t] - w[t];
}

}  // namespace amgx
