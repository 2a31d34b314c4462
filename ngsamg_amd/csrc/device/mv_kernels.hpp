// Multi-vector algebra kernels: the Gram matrix G = A^T B of two blocks of vectors and the update
// Y = beta Y + X c with a small host matrix c -- the two BLAS-3-shaped operations of a block eigensolver (LOBPCG / PINVIT:
// NGSolve's MultiVector.InnerProduct and MultiVector * matrix) next to amgx_matvec_multi and amgx_apply_multi.
//
// A multi-vector is addressed by two strides: entry (row r, column j) at r * rs + j * cs (column-major: rs = 1, cs = ld;
// interleaved: rs = k, cs = 1).
#pragma once

namespace amgx {

constexpr int MV_MAX = AMGX_MV_MAX;
constexpr int MV_BLOCKS = 1024;          // most workgroups (= partial Gram matrices) of one amgx_mv_gram
constexpr int MV_STAGE = 4096;           // doubles of a staged row chunk (all columns)
constexpr int MV_PF = MV_STAGE / BLOCK;  // ... per thread: the register copy of the next chunk
constexpr int MV_PAD = 2;                // LDS column stride = rows + 2 doubles: the operand reads of a wave (16 columns x 4 rows) hit 32 banks
typedef double mv_double4 __attribute__((ext_vector_type(4)));

// rows of a staged chunk for nc columns: the power of two in [64, 512] with rows * nc <= MV_STAGE
__host__ __device__ inline int mv_chunk_rows(int nc) {
  int rc = 512;
  while (rc > 64 && rc * nc > MV_STAGE) rc >>= 1;
  return rc;
}

// partial[(i * kb + j) * MV_BLOCKS + block] = sum over the rows of this workgroup's chunks of A[r][i] B[r][j].
//
// One pass over HBM for any ka, kb <= 32: a chunk of `rc` rows of ALL columns (A's, then B's; SYM: A's only) is staged in LDS,
// coalesced in either layout, while the previous chunk is multiplied; the ka x kb tile, padded to TA x TB tiles of 16 x 16, is
// accumulated by v_mfma_f64_16x16x4_f64 (operand layout as in dense_spd.hpp: A[m = lane & 15][k = lane >> 4], B[k][n = lane & 15],
// D[row = (lane >> 4) + 4 reg][col = lane & 15]) with the rows of the chunk as the contraction index: wave w takes the rows
// [w rc / 4, (w + 1) rc / 4) four at a time.  Lanes of padding columns feed 0.0, so a NaN of one column stays in its row and
// column of G.  SYM: only the tiles tb >= ta are computed.  Workgroup b takes the chunks b, b + gridDim.x, ...: the partial sums
// depend on (n, ka, kb, layout) alone.
template <int TA, int TB, bool SYM, bool IL>
__global__ __launch_bounds__(BLOCK) void mv_gram_kernel(int64_t n, int ka, int kb, const double* __restrict__ A, int64_t lda,
                                                        const double* __restrict__ B, int64_t ldb, int rc, double* __restrict__ partial) {
  extern __shared__ double mv_lds[];
  const int nc = SYM ? ka : ka + kb;
  const int st = rc + MV_PAD;
  const int total = rc * nc;                                   // <= MV_STAGE
  const int ea = rc * ka;                                      // staged elements of A
  const int lg = 31 - __clz(rc);
  const int tid = threadIdx.x;

  // element q of this thread: e = tid + q * BLOCK.  Column-major: e = col * rc + row (a column's rows are contiguous);
  // interleaved: A's rc x ka block, then B's rc x kb block, each contiguous in memory (e = row * k + col inside its block)
  auto lds_of = [&](int e) {
    if constexpr (IL) {
      const bool inb = e >= ea;
      const int k = inb ? kb : ka, f = inb ? e - ea : e;
      const int row = f / k, col = f - row * k;
      return ((inb ? ka : 0) + col) * st + row;
    } else {
      return (e >> lg) * st + (e & (rc - 1));
    }
  };
  int lds_il[IL ? MV_PF : 1];                                  // interleaved: kept (a division each); column-major: recomputed
  if constexpr (IL) {
#pragma unroll
    for (int q = 0; q < MV_PF; ++q) lds_il[q] = lds_of(min(tid + q * BLOCK, total - 1));
  }
  const int64_t n_chunks = (n + rc - 1) / rc;
  double pf[MV_PF];
  auto fetch = [&](int64_t chunk) {
    const int64_t r0 = chunk * rc;
#pragma unroll
    for (int q = 0; q < MV_PF; ++q) {
      const int e = tid + q * BLOCK;
      double v = 0.0;
      if (e < total) {
        if constexpr (IL) {
          const bool inb = e >= ea;
          const int k = inb ? kb : ka, f = inb ? e - ea : e;
          if (f < (n - r0) * k) v = (inb ? B : A)[r0 * k + f];  // (the block's elements inside the vectors)
        } else {
          const int c = e >> lg;
          const int64_t r = r0 + (e & (rc - 1));
          if (r < n) v = c < ka ? A[(int64_t)c * lda + r] : B[(int64_t)(c - ka) * ldb + r];
        }
      }
      pf[q] = v;
    }
  };
  auto stash = [&]() {
#pragma unroll
    for (int q = 0; q < MV_PF; ++q) {
      const int e = tid + q * BLOCK;
      if (e < total) {
        if constexpr (IL) mv_lds[lds_il[q]] = pf[q]; else mv_lds[lds_of(e)] = pf[q];
      }
    }
  };

  const int lane = tid & (WAVE - 1), w = tid >> 6;
  const int m = lane & 15, kq = lane >> 4;
  mv_double4 acc[TA][TB];
#pragma unroll
  for (int ta = 0; ta < TA; ++ta)
#pragma unroll
    for (int tb = 0; tb < TB; ++tb) acc[ta][tb] = mv_double4{0.0, 0.0, 0.0, 0.0};
  // operand columns of this lane (clamped: padding lanes read a valid address and feed 0.0)
  int ca[TA], cb[TB];
  bool va[TA], vb[TB];
#pragma unroll
  for (int ta = 0; ta < TA; ++ta) { const int c = 16 * ta + m; va[ta] = c < ka; ca[ta] = (va[ta] ? c : ka - 1) * st; }
#pragma unroll
  for (int tb = 0; tb < TB; ++tb) { const int c = 16 * tb + m; vb[tb] = c < kb; cb[tb] = ((SYM ? 0 : ka) + (vb[tb] ? c : kb - 1)) * st; }
  const int rows_w = rc >> 2;

  int64_t chunk = blockIdx.x;
  if (chunk < n_chunks) fetch(chunk);
  for (; chunk < n_chunks; chunk += gridDim.x) {
    __syncthreads();                                           // the previous chunk has been multiplied
    stash();
    __syncthreads();
    if (chunk + gridDim.x < n_chunks) fetch(chunk + gridDim.x);  // in flight while this chunk is multiplied
    for (int s = 0; s < rows_w; s += 4) {
      const int row = w * rows_w + s + kq;
      double a[TA], b[TB];
#pragma unroll
      for (int ta = 0; ta < TA; ++ta) { const double v = mv_lds[ca[ta] + row]; a[ta] = va[ta] ? v : 0.0; }
#pragma unroll
      for (int tb = 0; tb < TB; ++tb) { const double v = mv_lds[cb[tb] + row]; b[tb] = vb[tb] ? v : 0.0; }
#pragma unroll
      for (int ta = 0; ta < TA; ++ta)
#pragma unroll
        for (int tb = 0; tb < TB; ++tb)
          if (!SYM || tb >= ta) acc[ta][tb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[ta], b[tb], acc[ta][tb], 0, 0, 0);
    }
  }
  // the four waves' tiles, added in wave order
  __syncthreads();
  constexpr int TILE = TA * TB * 256;
#pragma unroll
  for (int ta = 0; ta < TA; ++ta)
#pragma unroll
    for (int tb = 0; tb < TB; ++tb)
#pragma unroll
      for (int r = 0; r < 4; ++r) mv_lds[w * TILE + (ta * TB + tb) * 256 + (kq + 4 * r) * 16 + m] = acc[ta][tb][r];
  __syncthreads();
  for (int e = tid; e < TILE; e += BLOCK) {
    const int t = e >> 8, ta = t / TB, tb = t - ta * TB;
    const int i = 16 * ta + ((e & 255) >> 4), j = 16 * tb + (e & 15);
    if (i >= ka || j >= kb || (SYM && tb < ta)) continue;
    double s = mv_lds[e];
#pragma unroll
    for (int q = 1; q < WAVES_PER_BLOCK; ++q) s += mv_lds[q * TILE + e];
    partial[(int64_t)(i * kb + j) * MV_BLOCKS + blockIdx.x] = s;
  }
}

// out[i * kb + j] = sum of the nb partials of the entry, in the fixed order and tree of kr_dot_final_kernel; one workgroup per
// entry.  sym: the entries of the tiles below the diagonal tiles are left alone (the host mirrors the upper triangle)
__global__ __launch_bounds__(BLOCK) void mv_gram_final_kernel(int nb, int kb, int sym, const double* __restrict__ partial, double* __restrict__ out) {
  __shared__ double red[BLOCK];
  const int i = blockIdx.x / kb, j = blockIdx.x - i * kb;
  if (sym && (j >> 4) < (i >> 4)) return;
  const double* p = partial + (int64_t)blockIdx.x * MV_BLOCKS;
  double acc = 0.0;
  for (int q = threadIdx.x; q < nb; q += BLOCK) acc += p[q];
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int o = BLOCK >> 1; o > 0; o >>= 1) { if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o]; __syncthreads(); }
  if (threadIdx.x == 0) out[blockIdx.x] = red[0];
}

// Y_j = beta Y_j + sum_i c[i][j] X_i, one row per thread: the kx entries of the row are read once, the ky sums live in
// registers (KYT >= ky of them, a compile-time count), c ([kx][KYT], zero-padded, in device memory) is read through uniform
// addresses.  Order per entry: beta * y first, then i ascending, fused multiply-add.  beta == 0: Y is not read.
template <int KYT>
__global__ __launch_bounds__(BLOCK) void mv_combine_kernel(int64_t n, int kx, int ky, const double* __restrict__ X, int64_t xrs, int64_t xcs,
                                                           const double* __restrict__ c, double beta, double* __restrict__ Y, int64_t yrs,
                                                           int64_t ycs) {
  const int64_t row = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (row >= n) return;
  double acc[KYT];
  double* __restrict__ yr = Y + row * yrs;
#pragma unroll
  for (int j = 0; j < KYT; ++j) acc[j] = (beta != 0.0 && j < ky) ? beta * yr[j * ycs] : 0.0;
  const double* __restrict__ xr = X + row * xrs;
  int i = 0;
  for (; i + 4 <= kx; i += 4) {
    const double x0 = xr[i * xcs], x1 = xr[(i + 1) * xcs], x2 = xr[(i + 2) * xcs], x3 = xr[(i + 3) * xcs];
    const double* __restrict__ ci = c + i * KYT;
#pragma unroll
    for (int j = 0; j < KYT; ++j) acc[j] = fma(ci[j], x0, acc[j]);
#pragma unroll
    for (int j = 0; j < KYT; ++j) acc[j] = fma(ci[KYT + j], x1, acc[j]);
#pragma unroll
    for (int j = 0; j < KYT; ++j) acc[j] = fma(ci[2 * KYT + j], x2, acc[j]);
#pragma unroll
    for (int j = 0; j < KYT; ++j) acc[j] = fma(ci[3 * KYT + j], x3, acc[j]);
  }
  for (; i < kx; ++i) {
    const double x0 = xr[i * xcs];
    const double* __restrict__ ci = c + i * KYT;
#pragma unroll
    for (int j = 0; j < KYT; ++j) acc[j] = fma(ci[j], x0, acc[j]);
  }
#pragma unroll
  for (int j = 0; j < KYT; ++j) if (j < ky) yr[j * ycs] = acc[j];
}

}  // namespace amgx
