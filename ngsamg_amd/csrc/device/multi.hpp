// Multi-vector apply path: k right-hand sides per matrix pass.
//
// Reference interface: BaseMatrix::Mult on an NGSolve MultiVector (what LOBPCG / PINVIT and callers with several load cases
// hand to a preconditioner); the reference runs AMGMatrix::Mult once per vector.  Here a handle whose smoothed levels are all
// scalar, plain Jacobi levels of a V-cycle runs the LITERAL cycle (x = w Dinv b, r = b - A x, b_c = P^T r, ..., t = x + P x_c,
// x = t + w Dinv (b - A t): amg_matrix.cpp:183-302) on the level images A, P, P^T with every matrix entry read ONCE for NV = 2 or 4
// vectors.  Inside the handle multi-vectors are interleaved, entry (row i, column j) at i*NV + j: a gathered column index
// then costs one address and 8*NV contiguous bytes.  Every other handle answers the same calls through a column loop over the
// single-vector path -- unless the call carries AMGX_MULTI_FUSE: then handles whose smoothed levels are plain
// Jacobi or Chebyshev levels with block size 1, 2, 3 or 6 run fused groups too (Multi::decide_extended; BSELL, block CSR and
// rigid-body kernels below, the Chebyshev recurrence of cheb_smooth per column).
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
  } else {
    // store_scalar<EP_CHEB> per column: d, y2 and yin interleaved like y
    static_assert(EP == EP_CHEB, "multi-vector epilogues: MULT, RES, AXPY, JAC, CHEB");
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
template <int K, bool C16, int NV, class V>
__device__ __forceinline__ void sell_consume_nv(const SellRegs<K, V>& R, const int32_t* __restrict__ cb, int r0, int p,
                                                const double* __restrict__ x, double (&acc0)[NV], double (&acc1)[NV]) {
  double x0[K][NV], x1[K][NV];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int q = p + k;
    const int c0 = C16 ? r0 + cb[2 * q] + (int)(R.ca[k] & 0xffffu) : (int)R.ca[k];
    const int c1 = C16 ? r0 + cb[2 * q + 1] + (int)(R.ca[k] >> 16) : (int)R.cb2[k];
    ldv<NV>(x + (int64_t)c0 * NV, x0[k]);
    ldv<NV>(x + (int64_t)c1 * NV, x1[k]);
  }
#pragma unroll
  for (int k = 0; k < K; ++k) {
#pragma unroll
    for (int j = 0; j < NV; ++j) { acc0[j] += (double)R.v0[k] * x0[k][j]; acc1[j] += (double)R.v1[k] * x1[k][j]; }
  }
}

template <int K, int REM, bool C16, int NV, class V>
__device__ __forceinline__ void sell_tail_nv(int rem, const SellRegs<K, V>* last, int p_last, const V* __restrict__ vb,
                                             const void* __restrict__ cpv, const int32_t* __restrict__ cb, int r0, int p, int lane,
                                             const double* __restrict__ x, double (&acc0)[NV], double (&acc1)[NV]) {
  if (rem == REM) {
    SellRegs<REM, V> R;
    sell_load<REM, C16>(R, vb, cpv, p, lane);
    if (last) sell_consume_nv<K, C16, NV>(*last, cb, r0, p_last, x, acc0, acc1);
    sell_consume_nv<REM, C16, NV>(R, cb, r0, p, x, acc0, acc1);
  } else if constexpr (REM > 1) sell_tail_nv<K, REM - 1, C16, NV, V>(rem, last, p_last, vb, cpv, cb, r0, p, lane, x, acc0, acc1);
}

template <bool C16, int NV, class V, int K = SELL_BATCH>
__device__ __forceinline__ void sell_pairs_nv(int np, const V* __restrict__ vb, const void* __restrict__ cpv, const int32_t* __restrict__ cb,
                                              int r0, int lane, const double* __restrict__ x, double (&acc0)[NV], double (&acc1)[NV]) {
  const int nfull = np / K, rem = np - nfull * K;
  if (nfull > 0) {
    SellRegs<K, V> A;
    sell_load<K, C16>(A, vb, cpv, 0, lane);
    for (int b = 1; b < nfull; ++b) {
      SellRegs<K, V> B;
      sell_load<K, C16>(B, vb, cpv, b * K, lane);
      sell_consume_nv<K, C16, NV>(A, cb, r0, (b - 1) * K, x, acc0, acc1);
      A = B;
    }
    if (K > 1 && rem) sell_tail_nv<K, (K > 1 ? K - 1 : 1), C16, NV, V>(rem, &A, (nfull - 1) * K, vb, cpv, cb, r0, nfull * K, lane, x, acc0, acc1);
    else sell_consume_nv<K, C16, NV>(A, cb, r0, (nfull - 1) * K, x, acc0, acc1);
  } else if (K > 1 && rem) sell_tail_nv<K, (K > 1 ? K - 1 : 1), C16, NV, V>(rem, nullptr, 0, vb, cpv, cb, r0, 0, lane, x, acc0, acc1);
}

// acc[j] = (SELL row of slice s, this lane) . column j of x          (sell_row_dot_sp for NV vectors)
template <int NV, class V>
__device__ __forceinline__ void sell_row_dot_nv(const SellMatT<V>& M, int s, int lane, int row, const double* __restrict__ x, double (&acc)[NV]) {
  const int64_t sp0 = M.slice_ptr[s], sp1 = M.slice_ptr[s + 1];
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
  if (c16) sell_pairs_nv<true, NV, V>(np, vb, M.col16 + base, cb, r0, lane, x, acc0, acc1);
  else sell_pairs_nv<false, NV, V>(np, vb, M.col32 + base, nullptr, 0, lane, x, acc0, acc1);
  if (w & 1) {
    const int c = c16 ? r0 + cb[w - 1] + cs : cs;
    double xs[NV];
    ldv<NV>(x + (int64_t)c * NV, xs);
#pragma unroll
    for (int j = 0; j < NV; ++j) acc0[j] += (double)vs * xs[j];
  }
#pragma unroll
  for (int j = 0; j < NV; ++j) acc[j] = acc0[j] + acc1[j];
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
template <int WB, int NV, int EP>
__global__ __launch_bounds__(WB) void sell_win_spmm_kernel(int64_t n_rows, SellMat M, const uint16_t* __restrict__ rowloc,
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
      for (int j = 0; j < NV; ++j) acc[j] += (double)v0 * xv[2 * cp][j] + (double)v1 * xv[2 * cp + 1][j];
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

// ---- element-wise pieces on interleaved vectors (one thread per entry) -------------------------------------------------------
// x = omega * Dinv * b, width 1 << sh      (diag_apply_kernel<1, false> per column)
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

// ---------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------

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

struct MultiWork {                      // work vectors of one fused width, kept from call to call
  struct Lev { DevBuf<double> x, rhs, res, tmp, d; };   // d: the update vector of a Chebyshev level
  std::vector<Lev> lev;
  DevBuf<double> in, out;               // interleaved copies of a group of the caller's columns (arguments that are not used in place)
};

struct MultiState {
  int fused = -1;                       // -1: not decided yet
  std::string why;                      // fused == 0: the first reason
  int fused_x = -1;                     // the same decision under AMGX_MULTI_FUSE (the extended rule)
  std::string why_x;
  MultiWork work[MULTI_MAX + 1];        // by width (2, 4)
  DevBuf<double> col_in, col_out;       // one contiguous column (single-vector path behind an interleaved argument)
  DevBuf<double> stage_b, stage_x;      // host-pointer calls
  DevBuf<double> kr[5];                 // amgx_pcg_multi: b, x, d, w, s (interleaved, width k)
  DevBuf<double> kr_sc, kr_partial;
  DevBuf<int32_t> kr_active;
  using Key = std::tuple<const double*, double*, int, int, int64_t, int64_t, int>;   // b, x, k, layout, ldb, ldx, extended rule in force
  GraphCache<Key> graphs;
};

void multi_drop_graphs(MultiState* s) { s->graphs.drop(); }       // amgx_set_stream: captures of the old stream go
void multi_free(MultiState* s) { delete s; }

struct Multi {
  Handle& h;
  MultiState& st;
  const bool fuse_flag;                 // the call carries AMGX_MULTI_FUSE
  const bool fz;                        // this call runs fused groups
  explicit Multi(Handle& hh, int flags = 0)
      : h(hh), st(state(hh)), fuse_flag(flags & AMGX_MULTI_FUSE), fz(st.fused == 1 || (fuse_flag && st.fused_x == 1)) {}
  bool extended() const { return fuse_flag && st.fused != 1; }     // the flag decides the path (a scalar Jacobi handle: one path, one graph)
  const std::string& note() const { return extended() ? st.why_x : st.why; }

  static MultiState& state(Handle& h) {
    if (!h.multi) h.multi = new MultiState;
    MultiState& s = *h.multi;
    if (s.fused < 0) { decide(h, s); decide_extended(h, s); }
    return s;
  }
  static bool spmm_ok(const DevMatrix& M) { return M.br == 1 && M.bc == 1 && (M.fmt == FMT_SELL || M.fmt == FMT_CSRVEC); }
  // all-or-nothing rule of the fused path: V-cycle; every smoothed level scalar, plain Jacobi, square, in the caller's numbering
  static void decide(Handle& h, MultiState& s) {
    s.fused = 0;
    const int L = h.n_levels();
    if (h.cycle != AMGX_CYCLE_V) { s.why = "cycle is not V"; return; }
    for (int l = 0; l < L; ++l) {
      const DevLevel& V = h.lev[l];
      const std::string at = " (level " + std::to_string(l) + ")";
      if (V.bs != 1) { s.why = "block level" + at; return; }
      if (V.n != V.ncols) { s.why = "ghost columns" + at; return; }
      if (h.permuted(l)) { s.why = "renumbered level" + at; return; }
      if (V.n > 0 && !spmm_ok(V.A)) { s.why = "level matrix format" + at; return; }
      if (l + 1 == L) break;
      if (V.sm_type != AMGX_SM_JACOBI) { s.why = "smoother is not Jacobi" + at; return; }
      if (!h.plain(V)) { s.why = "sm_steps > 1 or sm_symm" + at; return; }
      if (V.n > 0 && (!spmm_ok(V.P) || !spmm_ok(V.PT))) { s.why = "transfer format" + at; return; }
    }
    s.fused = 1;
  }

  // the extended rule (AMGX_MULTI_FUSE): Jacobi or Chebyshev per level, block sizes 1, 2, 3, 6, BSELL / block CSR level matrices,
  // rigid-body or block-CSR transfers.  A superset of decide(): fused == 1 implies fused_x == 1.
  static bool scalar_ok(const DevMatrix& M) { return M.fmt != FMT_RB && spmm_ok(M); }
  static bool bcsr_ok(const DevMatrix& M, bool square) {
    if (M.fmt != FMT_CSRVEC) return false;
    const int key = M.br * 10 + M.bc;
    if (square) return key == 22 || key == 33 || key == 66;
    return key == 22 || key == 33 || key == 66 || key == 36 || key == 63 || key == 23 || key == 32;
  }
  static bool level_ok(const DevMatrix& M) {
    if (M.br != M.bc) return false;
    if (M.br == 1) return scalar_ok(M);
    if (M.fmt == FMT_BSELL) return M.br == 2 || M.br == 3 || M.br == 6;
    return bcsr_ok(M, true);
  }
  static bool transfer_ok(const DevMatrix& M) { return M.fmt == FMT_RB || (M.br == 1 && M.bc == 1 ? scalar_ok(M) : bcsr_ok(M, false)); }
  static void decide_extended(Handle& h, MultiState& s) {
    s.fused_x = 0;
    const int L = h.n_levels();
    if (h.cycle != AMGX_CYCLE_V) { s.why_x = "cycle is not V"; return; }
    for (int l = 0; l < L; ++l) {
      const DevLevel& V = h.lev[l];
      const std::string at = " (level " + std::to_string(l) + ")";
      const bool smoothed = l + 1 < L;
      if (smoothed) {                                          // (the smoother first: it is the reason a caller can act on)
        if (V.sm_type != AMGX_SM_JACOBI && V.sm_type != AMGX_SM_CHEBY) { s.why_x = "smoother is not Jacobi or Chebyshev" + at; return; }
        if (!h.plain(V)) { s.why_x = "sm_steps > 1 or sm_symm" + at; return; }
        if (V.sm_type == AMGX_SM_CHEBY && (V.cheb_degree < 1 || V.cheb_degree > 8)) { s.why_x = "Chebyshev level without coefficients" + at; return; }
      }
      if (V.bs != 1 && V.bs != 2 && V.bs != 3 && V.bs != 6) { s.why_x = "block size is not 1, 2, 3 or 6" + at; return; }
      if (V.n != V.ncols) { s.why_x = "ghost columns" + at; return; }
      if (h.permuted(l)) { s.why_x = "renumbered level" + at; return; }
      if (V.n > 0 && (!level_ok(V.A) || V.A.br != V.bs)) { s.why_x = "level matrix format" + at; return; }
      if (smoothed && V.n > 0 && (!transfer_ok(V.P) || !transfer_ok(V.PT))) { s.why_x = "transfer format" + at; return; }
    }
    s.fused_x = 1;
  }

  // first level that the multi cycle hands to ONE dense product (collapsed operator or the coarsest level's inverse)
  // (0: the whole cycle is the dense operator, no level work vectors)
  int top() const { return h.dense_level >= 0 ? h.dense_level : h.n_levels() - 1; }

  int64_t work_bytes(int k) const {
    if (k == 1) return 0;                                       // amgx_apply itself
    int32_t wd[MULTI_MAX];
    const int ng = multi_groups(k, fz, wd);
    const int64_t n0 = h.lev[0].len();
    const int T = top();
    int64_t per_col = 2 * n0;                                  // the two interleaved copies of a group of the caller's columns
    for (int l = 0; l <= T && l < h.n_levels(); ++l)           // (a Chebyshev level: one more vector, the update d)
      per_col += ((l > 0 ? 2 : 0) + (l < T ? 2 + (h.lev[l].sm_type == AMGX_SM_CHEBY ? 1 : 0) : 0)) * h.lev[l].len();
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
    if (W.lev.empty()) {
      const int T = top();
      W.lev.resize(T + 1);
      for (int l = 0; l <= T; ++l) {
        const size_t len = (size_t)h.lev[l].len() * w;
        if (l > 0) { W.lev[l].x.alloc(len); W.lev[l].rhs.alloc(len); }
        if (l < T) { W.lev[l].res.alloc(len); W.lev[l].tmp.alloc(len); }
        if (l < T && h.lev[l].sm_type == AMGX_SM_CHEBY) W.lev[l].d.alloc(len);
      }
    }
    return W;
  }

  // ------------------------------------------------------------------ launches
  // sm_pass: a product of the cycle on a level (EP_CHEB steps, the residual after smoothing): it reads the single-precision image
  // where the level has one, as Handle::spmv_ep does; amgx_matvec_multi and the level-0 product of amgx_pcg_multi never pass it.
  template <int NV, int EP>
  void spmm_nv(const DevMatrix& M, const double* x, double* y, const EpArgs& ep, bool sm_pass = false) {
    if (M.n_rows == 0) return;
    hipStream_t s = h.stream;
    if constexpr (EP == EP_RES || EP == EP_CHEB) {
      if (sm_pass && M.has32()) { spmm_nv32<NV, EP>(M, x, y, ep); return; }
    }
    if (M.fmt == FMT_RB) {
      if constexpr (EP != EP_MULT && EP != EP_AXPY) throw Err("rigid-body transfer blocks: y = M x and y = yin + s M x only");
      else {
        const DevMatrix::Rb& R = M.rb;
        const RbMat V = R.view();
        auto run = [&](auto BF, auto BC, auto DM) {            // shapes and lanes per coarse row as in Handle::spmv_ep
          constexpr int G = 16;
          if (!R.transposed) launch(rb_prolong_nv_kernel<BF(), BC(), DM(), NV, EP>, Handle::grid_for(M.n_rows), BLOCK, 0, s, M.n_rows, V, x, y, ep);
          else launch(rb_restrict_nv_kernel<BF(), BC(), DM(), G, NV, EP>, Handle::grid_for(M.n_rows * G), BLOCK, 0, s, M.n_rows, V, x, y, ep);
        };
        if (R.dim == 3 && R.bf == 6) run(Int<6>{}, Int<6>{}, Int<3>{});
        else if (R.dim == 3) run(Int<3>{}, Int<6>{}, Int<3>{});
        else if (R.dim == 2 && R.bf == 3) run(Int<3>{}, Int<3>{}, Int<2>{});
        else if (R.dim == 2) run(Int<2>{}, Int<3>{}, Int<2>{});
        else run(Int<2>{}, Int<2>{}, Int<0>{});
      }
    } else if (M.fmt == FMT_SELL && M.sell.win) {
      if (M.sell.win != SELL_WIN) throw Err("windowed SELL: unexpected window size");
      const int nw = (int)((M.n_rows + SELL_WIN - 1) / SELL_WIN);
      launch(sell_win_spmm_kernel<SELL_WIN, NV, EP>, nw, SELL_WIN, 0, s, M.n_rows, M.sell.view(), M.sell.rowloc.p, x, y, ep);
    } else if (M.fmt == FMT_SELL) {
      const int grid = (M.n_slices + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK;
      auto run = [&](auto G) { launch(sell_spmm_kernel<G(), NV, EP>, grid, BLOCK, 0, s, M.n_rows, M.n_slices, M.sell.view(), x, y, ep); };
      if (!dispatch<1, 2, 4, 8>(M.lanes, run)) run(Int<16>{});       // any other lane count: the 16-lane kernel
    } else if (M.fmt == FMT_CSRVEC && M.br == 1 && M.bc == 1) {
      const int grid = Handle::grid_for(M.n_rows * M.lanes);
      auto run = [&](auto G) { launch(csrvec_spmm_kernel<G(), NV, EP>, grid, BLOCK, 0, s, M.n_rows, M.rowptr.p, M.col.p, M.val.p, x, y, ep); };
      if (!dispatch<2, 4, 8, 16, 32>(M.lanes, run)) run(Int<64>{});  // any other lane count: one wave per row
    } else if (M.fmt == FMT_BSELL) {
      const int grid = (M.n_slices + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK;
      auto run = [&](auto BS) { launch(bsell_spmm_kernel<BS(), NV, EP>, grid, BLOCK, 0, s, M.n_rows, M.n_slices, M.bsell.view(0), x, y, ep); };
      if (!dispatch<6, 3, 2>(M.br, run)) throw Err("multi-vector product: unsupported BSELL block size");
    } else if (M.fmt == FMT_CSRVEC) {
      constexpr int W = 4;
      auto run = [&](auto KEY) {                                     // key = 10 * br + bc
        constexpr int BR = KEY() / 10, BC = KEY() % 10;
        const int rpw = WAVE / (BR * W);
        const int64_t waves = (M.n_rows + rpw - 1) / rpw;
        const int grid = (int)std::max<int64_t>(1, (waves + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK);
        launch(bcsr_spmm_kernel<BR, BC, NV, EP, W>, grid, BLOCK, 0, s, M.n_rows, M.rowptr.p, M.col.p, M.val.p, x, y, ep);
      };
      const int key = M.br * 10 + M.bc;
      bool ok;
      if constexpr (EP == EP_JAC || EP == EP_CHEB) ok = dispatch<22, 33, 66>(key, run);
      else ok = dispatch<22, 33, 66, 36, 63, 23, 32>(key, run);
      if (!ok) throw Err("multi-vector product: unsupported block shape " + std::to_string(M.br) + "x" + std::to_string(M.bc));
    } else throw Err("multi-vector product: matrix format has no multi-vector kernel");
  }
  // the smoother passes on the single-precision image (Handle::spmv_ep32)
  template <int NV, int EP>
  void spmm_nv32(const DevMatrix& M, const double* x, double* y, const EpArgs& ep) {
    hipStream_t s = h.stream;
    if (M.fmt == FMT_SELL && !M.sell.win) {
      const int grid = (M.n_slices + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK;
      auto run = [&](auto G) { launch(sell_spmm_kernel<G(), NV, EP, float>, grid, BLOCK, 0, s, M.n_rows, M.n_slices, M.sell.view32(M.val32.p), x, y, ep); };
      if (!dispatch<1, 2, 4, 8>(M.lanes, run)) run(Int<16>{});
    } else if (M.fmt == FMT_BSELL) {
      const int grid = (M.n_slices + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK;
      const BSellMatT<float> V = M.bsell.view32(M.val32.p, 0);
      auto run = [&](auto BS) { launch(bsell_spmm_kernel<BS(), NV, EP, float>, grid, BLOCK, 0, s, M.n_rows, M.n_slices, V, x, y, ep); };
      if (!dispatch<6, 3, 2>(M.br, run)) throw Err("single-precision image: unsupported block size");
    } else throw Err("single-precision image on a format that has none");
  }
  template <int EP>
  void spmm(int w, const DevMatrix& M, const double* x, double* y, const EpArgs& ep, bool sm_pass = false) {
    if (w == 2) spmm_nv<2, EP>(M, x, y, ep, sm_pass);
    else if (w == 4) spmm_nv<4, EP>(M, x, y, ep, sm_pass);
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
    const int grid = (n + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK;
    auto run = [&](auto W) { launch(dense_gemm_nv_kernel<W()>, grid, BLOCK, 0, h.stream, n, ld, M, x, y); };
    if (!dispatch<2, 4>(w, run)) throw Err("multi-vector dense product: width must be 2 or 4");
  }
  void pack(int64_t n, int w, const double* src, int64_t rs, int64_t cs, int c0, double* dst) {
    if (n <= 0) return;
    launch(multi_pack_kernel, Handle::grid_for(n * w), BLOCK, 0, h.stream, n, w, src, rs, cs, c0, dst);
  }
  void unpack(int64_t n, int w, const double* src, double* dst, int64_t rs, int64_t cs, int c0) {
    if (n <= 0) return;
    launch(multi_unpack_kernel, Handle::grid_for(n * w), BLOCK, 0, h.stream, n, w, src, dst, rs, cs, c0);
  }

  void coarse_multi(int w, const double* rhs, double* x) {
    const DevLevel& V = h.lev.back();
    if (h.clev != AMGX_CLEV_INV || h.coarse_n == 0) { h.zero(x, V.len() * w); return; }
    gemm(w, (int)h.coarse_n, (int)h.coarse_ld, h.coarse_inv.p, rhs, x);
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
      if (V.sm_type == AMGX_SM_CHEBY) {
        // cheb_smooth from zero per column: step 1 without a product (d == x), steps 2 .. k out of place between x and tmp,
        // started where the last one ends in x
        const int k = V.cheb_degree;
        double* cur = ((k - 1) & 1) ? tmp : xl;
        diag(w, V, bl, cur, V.cheb_c0);
        const double* dcur = nullptr;
        for (int j = 2; j <= k; ++j) {
          double* nxt = cur == xl ? tmp : xl;
          spmm<EP_CHEB>(w, V.A, cur, nxt, EpArgs{bl, cur, V.dinv.p, V.cheb_c2[j], j < k ? W.lev[l].d.p : nullptr, 0, dcur, V.cheb_c1[j]}, true);
          dcur = W.lev[l].d.p;
          cur = nxt;
        }
      } else diag(w, V, bl, xl, V.omega);
      spmm<EP_RES>(w, V.A, xl, W.lev[l].res.p, EpArgs{bl, nullptr, nullptr, 0.0, nullptr, 0}, true);
      spmm<EP_MULT>(w, V.PT, W.lev[l].res.p, W.lev[l + 1].rhs.p, none);
    }
    if (h.dense_level > 0) gemm(w, h.dense_n, h.dense_ld, h.dense_op.p, W.lev[T].rhs.p, W.lev[T].x.p);
    else coarse_multi(w, W.lev[T].rhs.p, W.lev[T].x.p);
    for (int l = T - 1; l >= 0; --l) {
      const DevLevel& V = h.lev[l];
      double* xl = l == 0 ? x : W.lev[l].x.p;
      const double* bl = l == 0 ? b : W.lev[l].rhs.p;
      double* const tmp = W.lev[l].tmp.p;
      if (V.sm_type == AMGX_SM_CHEBY) {
        // k out-of-place steps follow: t = x + P x_c goes where an even number of them is left before x (in place when k is even)
        const int k = V.cheb_degree;
        double* cur = (k & 1) ? tmp : xl;
        spmm<EP_AXPY>(w, V.P, W.lev[l + 1].x.p, cur, EpArgs{nullptr, xl, nullptr, 1.0, nullptr, 0});
        const double* dcur = nullptr;
        for (int j = 1; j <= k; ++j) {                         // (step 1: (c1, c2) = (0, c0), d_old = nullptr)
          double* nxt = cur == xl ? tmp : xl;
          const double c1 = j == 1 ? 0.0 : V.cheb_c1[j], c2 = j == 1 ? V.cheb_c0 : V.cheb_c2[j];
          spmm<EP_CHEB>(w, V.A, cur, nxt, EpArgs{bl, cur, V.dinv.p, c2, j < k ? W.lev[l].d.p : nullptr, 0, dcur, c1}, true);
          dcur = W.lev[l].d.p;
          cur = nxt;
        }
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

  // X = C B on device multi-vectors; (rs, cs) strides of B / X: entry (i, j) at i*rs + j*cs
  void apply_body(int k, const double* B, int64_t brs, int64_t bcs, double* X, int64_t xrs, int64_t xcs, bool graph_ok, bool capturing) {
    const int64_t n = h.lev[0].len();
    int32_t wd[MULTI_MAX];
    const int ng = multi_groups(k, fz, wd);
    int c0 = 0;
    for (int g = 0; g < ng; c0 += wd[g], ++g) {
      const int w = wd[g];
      if (w == 1) {
        const double* b1 = B + c0 * bcs;
        double* x1 = X + c0 * xcs;
        if (brs != 1) { fit(st.col_in, n); pack(n, 1, B, brs, bcs, c0, st.col_in.p); b1 = st.col_in.p; }
        if (xrs != 1) { fit(st.col_out, n); x1 = st.col_out.p; }
        apply_single(b1, x1, graph_ok, capturing);
        if (xrs != 1) unpack(n, 1, st.col_out.p, X, xrs, xcs, c0);
        continue;
      }
      MultiWork& W = work(w);
      // interleaved arguments of exactly this width (16-byte aligned) are used in place
      const bool b_inplace = brs == w && bcs == 1 && k == w && (reinterpret_cast<uintptr_t>(B) & 15) == 0;
      const bool x_inplace = xrs == w && xcs == 1 && k == w && (reinterpret_cast<uintptr_t>(X) & 15) == 0;
      const double* bw = B;
      double* xw = X;
      if (!b_inplace) { fit(W.in, n * w); pack(n, w, B, brs, bcs, c0, W.in.p); bw = W.in.p; }
      if (!x_inplace) { fit(W.out, n * w); xw = W.out.p; }
      cycle_v_multi(w, xw, bw);
      if (!x_inplace) unpack(n, w, W.out.p, X, xrs, xcs, c0);
    }
  }

  void apply(int k, const double* B, int64_t ldb, double* X, int64_t ldx, bool interleaved, bool graph_ok) {
    const int64_t brs = interleaved ? k : 1, bcs = interleaved ? 1 : ldb, xrs = interleaved ? k : 1, xcs = interleaved ? 1 : ldx;
    // only the fused path is captured as a whole; the column loop replays the single-vector graphs of run_cycle
    if (!fz || !(h.use_graph && graph_ok) || h.stream == nullptr) { apply_body(k, B, brs, bcs, X, xrs, xcs, graph_ok, false); return; }
    const MultiState::Key key{B, X, k, interleaved ? 1 : 0, interleaved ? 0 : ldb, interleaved ? 0 : ldx, extended() ? 1 : 0};
    if (!st.graphs.has(key)) {
      int32_t wd[MULTI_MAX];
      const int ng = multi_groups(k, true, wd);
      for (int g = 0; g < ng; ++g) {                           // allocations happen before the capture
        if (wd[g] > 1) { MultiWork& W = work(wd[g]); fit(W.in, h.lev[0].len() * wd[g]); fit(W.out, h.lev[0].len() * wd[g]); }
        else { fit(st.col_in, h.lev[0].len()); fit(st.col_out, h.lev[0].len()); }
      }
    }
    st.graphs.run(key, h.stream, [&] { apply_body(k, B, brs, bcs, X, xrs, xcs, false, true); });
  }

  // Y = A_level X on device multi-vectors
  void matvec(int level, int k, const double* X, int64_t ldx, double* Y, int64_t ldy, bool interleaved) {
    const DevLevel& V = h.lev[level];
    const int64_t n = V.len(), nx = V.ext_len();
    const int64_t xrs = interleaved ? k : 1, xcs = interleaved ? 1 : ldx, yrs = interleaved ? k : 1, ycs = interleaved ? 1 : ldy;
    int32_t wd[MULTI_MAX];
    const int ng = multi_groups(k, fz, wd);
    int c0 = 0;
    for (int g = 0; g < ng; c0 += wd[g], ++g) {
      const int w = wd[g];
      if (w == 1) {                                            // amgx_matvec with device pointers
        const double* x1 = X + c0 * xcs;
        double* y1 = Y + c0 * ycs;
        if (xrs != 1) { fit(st.col_in, std::max(nx, h.lev[0].len())); pack(nx, 1, X, xrs, xcs, c0, st.col_in.p); x1 = st.col_in.p; }
        if (yrs != 1) { fit(st.col_out, std::max(n, h.lev[0].len())); y1 = st.col_out.p; }
        Staged sg(h, AMGX_DEVICE_PTR);
        const double* dx = sg.in(0, x1, nx, level);
        double* dy = sg.inout(1, y1, n, false, level);
        h.mult(V.A, dx, dy);
        sg.out(1, y1, n, level);
        if (yrs != 1) unpack(n, 1, st.col_out.p, Y, yrs, ycs, c0);
        continue;
      }
      MultiWork& W = work(w);
      const bool x_inplace = xrs == w && xcs == 1 && k == w && (reinterpret_cast<uintptr_t>(X) & 15) == 0;
      const bool y_inplace = yrs == w && ycs == 1 && k == w && (reinterpret_cast<uintptr_t>(Y) & 15) == 0;
      const double* xw = X;
      double* yw = Y;
      // (the interleaved copies are sized for level 0, the largest level)
      if (!x_inplace) { fit(W.in, h.lev[0].len() * w); pack(n, w, X, xrs, xcs, c0, W.in.p); xw = W.in.p; }
      if (!y_inplace) { fit(W.out, h.lev[0].len() * w); yw = W.out.p; }
      spmm<EP_MULT>(w, V.A, xw, yw, EpArgs{nullptr, nullptr, nullptr, 0.0, nullptr, 0});      // (no sm_pass: the fp64 image)
      if (!y_inplace) unpack(n, w, W.out.p, Y, yrs, ycs, c0);
    }
  }

  // k independent preconditioned CG recurrences (Krylov::pcg per column) that share the operator product and the preconditioner
  // application.  B, X: device multi-vectors (strides as apply_body).
  void pcg(int k, const double* B, int64_t brs, int64_t bcs, double* X, int64_t xrs, int64_t xcs, double tol, int maxit, bool use_pre,
           bool graph_ok, double* errs, int32_t* iters) {
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
    pack(n, k, B, brs, bcs, 0, b);
    pack(n, k, X, xrs, xcs, 0, x);
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
    unpack(n, k, x, X, xrs, xcs, 0);
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

inline void multi_check(const char* fn, int k, const void* a, const void* b, int64_t lda, int64_t ldb, int64_t rows_a, int64_t rows_b, bool interleaved) {
  const std::string f(fn);
  if (k < 1 || k > MULTI_MAX) throw Err(f + ": k must be 1 .. " + std::to_string(MULTI_MAX) + " (got " + std::to_string(k) + ")");
  if (!a || !b) throw Err(f + ": null multi-vector");
  if (a == b) throw Err(f + ": the multi-vectors must not alias");
  if (!interleaved && k > 1 && (lda < rows_a || ldb < rows_b)) throw Err(f + ": leading dimension below the level size");
}

}  // namespace amgx

extern "C" {

int amgx_apply_multi(amgx_handle hh, int k, const double* B, int64_t ldb, double* X, int64_t ldx, int b_status, int flags) {
  if (k == 1 && hh && hh->h) return amgx_apply(hh, B, X, b_status, flags & ~(AMGX_MULTI_INTERLEAVED | AMGX_MULTI_FUSE));   // the single-vector path itself
  (void)b_status;   // single GPU: DISTRIBUTED == CUMULATED, as in amgx_apply
  return guard(hh, [&](amgx::Handle& h) {
    const int64_t n = h.lev[0].len();
    const bool il = flags & AMGX_MULTI_INTERLEAVED;
    amgx::multi_check("amgx_apply_multi", k, B, X, ldb, ldx, n, n, il);
    amgx::Multi M(h, flags);
    amgx::MultiStaged sg(h, flags);
    const int64_t lb = (sg.host && !il) ? n : ldb, lx = (sg.host && !il) ? n : ldx;      // (staged copies are compact)
    const double* dB = sg.in(M.st.stage_b, B, n, k, il, ldb);
    double* dX = const_cast<double*>(sg.in(M.st.stage_x, X, n, k, il, ldx, false));
    M.apply(k, dB, lb, dX, lx, il, !(flags & AMGX_NO_GRAPH));
    sg.out(M.st.stage_x, X, n, k, il, ldx);
  });
}

int amgx_matvec_multi(amgx_handle hh, int level, int k, const double* X, int64_t ldx, double* Y, int64_t ldy, int flags) {
  return guard(hh, [&](amgx::Handle& h) {
    if (level < 0 || level >= h.n_levels()) throw amgx::Err("amgx_matvec_multi: level out of range");
    const int64_t n = h.lev[level].len(), nx = h.lev[level].ext_len();
    const bool il = flags & AMGX_MULTI_INTERLEAVED;
    amgx::multi_check("amgx_matvec_multi", k, X, Y, ldx, ldy, nx, n, il);
    amgx::Multi M(h, flags);
    amgx::MultiStaged sg(h, flags);
    const int64_t lx = (sg.host && !il) ? nx : ldx, ly = (sg.host && !il) ? n : ldy;
    const double* dX = sg.in(M.st.stage_b, X, nx, k, il, ldx);
    double* dY = const_cast<double*>(sg.in(M.st.stage_x, Y, n, k, il, ldy, false));
    M.matvec(level, k, dX, lx, dY, ly, il);
    sg.out(M.st.stage_x, Y, n, k, il, ldy);
  });
}

int amgx_pcg_multi(amgx_handle hh, int k, const double* B, int64_t ldb, double* X, int64_t ldx, double tol, int maxit, int use_precond, int flags,
                   double* errs, int32_t* iters) {
  return guard(hh, [&](amgx::Handle& h) {
    const int64_t n = h.lev[0].len();
    const bool il = flags & AMGX_MULTI_INTERLEAVED;
    amgx::multi_check("amgx_pcg_multi", k, B, X, ldb, ldx, n, n, il);
    if (maxit < 0 || !iters) throw amgx::Err("amgx_pcg_multi: bad arguments (maxit < 0 or iters == NULL)");
    amgx::Multi M(h, flags);
    amgx::MultiStaged sg(h, flags);
    const int64_t lb = (sg.host && !il) ? n : ldb, lx = (sg.host && !il) ? n : ldx;
    const double* dB = sg.in(M.st.stage_b, B, n, k, il, ldb);
    double* dX = const_cast<double*>(sg.in(M.st.stage_x, X, n, k, il, ldx));
    M.pcg(k, dB, il ? k : 1, il ? 1 : lb, dX, il ? k : 1, il ? 1 : lx, tol, maxit, use_precond != 0, !(flags & AMGX_NO_GRAPH), errs, iters);
    sg.out(M.st.stage_x, X, n, k, il, ldx);
  });
}

int amgx_multi_info(amgx_handle hh, int k, int32_t* fused, int32_t* n_groups, int32_t* group_width, int64_t* work_bytes) {
  return amgx_multi_plan(hh, k, 0, fused, n_groups, group_width, work_bytes);
}

int amgx_multi_plan(amgx_handle hh, int k, int flags, int32_t* fused, int32_t* n_groups, int32_t* group_width, int64_t* work_bytes) {
  return guard(hh, [&](amgx::Handle& h) {
    const std::string fn = (flags & AMGX_MULTI_FUSE) ? "amgx_multi_plan" : "amgx_multi_info";
    if (k < 1 || k > amgx::MULTI_MAX) throw amgx::Err(fn + ": k must be 1 .. " + std::to_string(amgx::MULTI_MAX) + " (got " + std::to_string(k) + ")");
    amgx::Multi M(h, flags & AMGX_MULTI_FUSE);
    int32_t wd[amgx::MULTI_MAX];
    const int ng = amgx::multi_groups(k, M.fz, wd);
    if (fused) *fused = M.fz ? 1 : 0;
    if (n_groups) *n_groups = ng;
    if (group_width) for (int g = 0; g < amgx::MULTI_MAX; ++g) group_width[g] = g < ng ? wd[g] : 0;
    if (work_bytes) *work_bytes = M.work_bytes(k);
  });
}

const char* amgx_multi_note(amgx_handle hh, int flags) {
  thread_local std::string note;
  note.clear();
  if (guard(hh, [&](amgx::Handle& h) {
        amgx::Multi M(h, flags & AMGX_MULTI_FUSE);
        if (!M.fz) note = M.note();
      }))
    note = amgx_last_error(hh);
  return note.c_str();
}

}  // extern "C"
