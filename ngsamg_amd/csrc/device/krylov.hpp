// Device-resident Krylov solvers around the preconditioner: preconditioned CG and restarted GMRES with
// hand-written BLAS-1 kernels -- the callers of the hot path on the reference side are NGSolve's CGSolver / GMRes
// (reference tests/h1/amg_utils.py:346, ngsolve.krylovspace); with the vectors resident in HBM one iteration is the
// preconditioner application + one SpMV + a few fused vector passes, and the host only reads one scalar per iteration.
//
// Reductions are deterministic: a fixed grid of workgroups writes partial sums, one workgroup adds them in a fixed order.
// The scalars of the recurrences (alpha, beta) stay on the device; kernels read them from memory.
#pragma once
#include "krylov_core.hpp"       // pcg, pcg_sr, gmres over a space; the SR_* scalar slots

namespace amgx {

// partial[blockIdx.x + slot * KR_BLOCKS] = sum over this block's grid-stride share of a[i] * b[i]
__global__ __launch_bounds__(BLOCK) void kr_dot_partial_kernel(int64_t n, const double* __restrict__ a, const double* __restrict__ b,
                                                               double* __restrict__ partial) {
  __shared__ double red[BLOCK / WAVE];
  double acc = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * BLOCK) acc += a[i] * b[i];
#pragma unroll
  for (int o = WAVE >> 1; o > 0; o >>= 1) acc += __shfl_xor(acc, o, WAVE);
  if ((threadIdx.x & (WAVE - 1)) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) { double s = 0.0; for (int w = 0; w < BLOCK / WAVE; ++w) s += red[w]; partial[blockIdx.x] = s; }
}
// several dot products against one vector in one pass: partial[j * KR_BLOCKS + block] = <V_j, w> share (Arnoldi: h = V^T w)
__global__ __launch_bounds__(BLOCK) void kr_multi_dot_partial_kernel(int64_t n, int m, const double* __restrict__ V, int64_t ldv,
                                                                     const double* __restrict__ w, double* __restrict__ partial) {
  __shared__ double red[BLOCK / WAVE];
  for (int j = 0; j < m; ++j) {
    const double* __restrict__ v = V + (int64_t)j * ldv;
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * BLOCK) acc += v[i] * w[i];
#pragma unroll
    for (int o = WAVE >> 1; o > 0; o >>= 1) acc += __shfl_xor(acc, o, WAVE);
    if ((threadIdx.x & (WAVE - 1)) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) { double s = 0.0; for (int q = 0; q < BLOCK / WAVE; ++q) s += red[q]; partial[(int64_t)j * KR_BLOCKS + blockIdx.x] = s; }
    __syncthreads();
  }
}
// out[j] = sum of the nb partials of product j, fixed order; one workgroup per product
__global__ __launch_bounds__(BLOCK) void kr_dot_final_kernel(int nb, const double* __restrict__ partial, double* __restrict__ out) {
  __shared__ double red[BLOCK];
  const double* p = partial + (int64_t)blockIdx.x * KR_BLOCKS;
  double acc = 0.0;
  for (int i = threadIdx.x; i < nb; i += BLOCK) acc += p[i];
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int o = BLOCK >> 1; o > 0; o >>= 1) { if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o]; __syncthreads(); }
  if (threadIdx.x == 0) out[blockIdx.x] = red[0];
}
// dot product in ONE launch (the CG recurrences: 7 -> 5 launches per iteration next to the cycle): every workgroup leaves its
// partial sum, takes a ticket, and the workgroup that draws the last one adds the partials exactly as kr_dot_final_kernel does
// (same order, same tree: the same bits) and re-arms the ticket counter
__global__ __launch_bounds__(BLOCK) void kr_dot_kernel(int64_t n, const double* __restrict__ a, const double* __restrict__ b,
                                                       double* __restrict__ partial, unsigned int* __restrict__ ticket, double* __restrict__ out) {
  __shared__ double red[BLOCK];
  __shared__ bool last;
  double acc = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * BLOCK) acc += a[i] * b[i];
#pragma unroll
  for (int o = WAVE >> 1; o > 0; o >>= 1) acc += __shfl_xor(acc, o, WAVE);
  if ((threadIdx.x & (WAVE - 1)) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int w = 0; w < BLOCK / WAVE; ++w) s += red[w];
    __hip_atomic_store(partial + blockIdx.x, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __threadfence();
    last = atomicAdd(ticket, 1u) == gridDim.x - 1;
  }
  __syncthreads();
  if (!last) return;
  __threadfence();
  const int nb = (int)gridDim.x;
  double t = 0.0;
  for (int i = threadIdx.x; i < nb; i += BLOCK) t += __hip_atomic_load(partial + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  red[threadIdx.x] = t;
  __syncthreads();
  for (int o = BLOCK >> 1; o > 0; o >>= 1) { if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o]; __syncthreads(); }
  if (threadIdx.x == 0) { out[0] = red[0]; *ticket = 0u; }
}
// CG update with alpha = sc[num] / sc[den] read on the device: x += alpha s, d -= alpha q
__global__ __launch_bounds__(BLOCK) void kr_cg_update_kernel(int64_t n, const double* __restrict__ sc, int num, int den,
                                                             const double* __restrict__ s, const double* __restrict__ q,
                                                             double* __restrict__ x, double* __restrict__ d) {
  const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  const double alpha = sc[num] / sc[den];
  x[i] += alpha * s[i];
  d[i] -= alpha * q[i];
}
// s = w + beta s, beta = sc[num] / sc[den]
__global__ __launch_bounds__(BLOCK) void kr_xpby_kernel(int64_t n, const double* __restrict__ sc, int num, int den,
                                                        const double* __restrict__ w, double* __restrict__ s) {
  const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  s[i] = w[i] + (sc[num] / sc[den]) * s[i];
}
// w -= sum_j h[j] V_j (Gram-Schmidt), one pass over w
__global__ __launch_bounds__(BLOCK) void kr_multi_axpy_kernel(int64_t n, int m, const double* __restrict__ V, int64_t ldv,
                                                              const double* __restrict__ h, double sign, double* __restrict__ w) {
  const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  double acc = w[i];
  for (int j = 0; j < m; ++j) acc += sign * h[j] * V[(int64_t)j * ldv + i];
  w[i] = acc;
}
// y = a * x   /   y += a * x with a host scalar
__global__ __launch_bounds__(BLOCK) void kr_scale_kernel(int64_t n, double a, const double* __restrict__ x, double* __restrict__ y, int add) {
  const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i < n) y[i] = (add ? y[i] : 0.0) + a * x[i];
}

// ---- single-reduction PCG (Chronopoulos / Gear form of the same recurrence): ONE reduction point per iteration -------------
// gamma = <r, u>, delta = <w, u> with u = C r, w = A u in one pass; partial[blk] / partial[KR_BLOCKS + blk]
__global__ __launch_bounds__(BLOCK) void kr_dot2_partial_kernel(int64_t n, const double* __restrict__ r, const double* __restrict__ u,
                                                                const double* __restrict__ w, double* __restrict__ partial) {
  __shared__ double red[2][BLOCK / WAVE];
  double a = 0.0, c = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * BLOCK) { const double ui = u[i]; a += r[i] * ui; c += w[i] * ui; }
#pragma unroll
  for (int o = WAVE >> 1; o > 0; o >>= 1) { a += __shfl_xor(a, o, WAVE); c += __shfl_xor(c, o, WAVE); }
  if ((threadIdx.x & (WAVE - 1)) == 0) { red[0][threadIdx.x >> 6] = a; red[1][threadIdx.x >> 6] = c; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double s0 = 0.0, s1 = 0.0;
    for (int q = 0; q < BLOCK / WAVE; ++q) { s0 += red[0][q]; s1 += red[1][q]; }
    partial[blockIdx.x] = s0;
    partial[KR_BLOCKS + blockIdx.x] = s1;
  }
}
// sc[SR_GNEW], sc[SR_DELTA] = sums of the n_local x KR_BLOCKS partials of the two products (fixed order); two workgroups
__global__ __launch_bounds__(BLOCK) void kr_sr_reduce_kernel(int n_local, const double* __restrict__ partial, double* __restrict__ sc) {
  __shared__ double red[BLOCK];
  const int j = blockIdx.x;                    // 0: gamma, 1: delta
  double acc = 0.0;
  for (int i = 0; i < n_local; ++i) {
    const double* p = partial + ((size_t)i * 2 + j) * KR_BLOCKS;
    for (int q = threadIdx.x; q < KR_BLOCKS; q += BLOCK) acc += p[q];
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int o = BLOCK >> 1; o > 0; o >>= 1) { if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o]; __syncthreads(); }
  if (threadIdx.x == 0) sc[SR_GNEW + j] = red[0];
}
// beta = gamma_new / gamma_old (0 on the first pass), alpha = gamma_new / (delta - beta * gamma_new / alpha_old); gamma_old <- gamma_new
__global__ void kr_sr_scalars_kernel(double* __restrict__ sc) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const double g = sc[SR_GNEW], d = sc[SR_DELTA];
  const bool first = sc[SR_FIRST] != 0.0;
  const double beta = first ? 0.0 : g / sc[SR_GOLD];
  const double alpha = first ? g / d : g / (d - beta * g / sc[SR_ALPHA]);
  sc[SR_BETA] = beta; sc[SR_ALPHA] = alpha; sc[SR_GOLD] = g; sc[SR_FIRST] = 0.0;
}
// p = u + beta p; s = w + beta s; x += alpha p; r -= alpha s      (one pass: 6 reads, 4 writes)
__global__ __launch_bounds__(BLOCK) void kr_sr_update_kernel(int64_t n, const double* __restrict__ sc, const double* __restrict__ u,
                                                             const double* __restrict__ w, double* __restrict__ p, double* __restrict__ s,
                                                             double* __restrict__ x, double* __restrict__ r) {
  const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  const double alpha = sc[SR_ALPHA], beta = sc[SR_BETA];
  const double pi = u[i] + beta * p[i], si = w[i] + beta * s[i];
  p[i] = pi; s[i] = si;
  x[i] += alpha * pi;
  r[i] -= alpha * si;
}

// The single-rank space of krylov_core.hpp: one pointer per vector, the operator and the cycle of one handle, every sum in one
// ticketed launch.  Built per solve (its constructor re-arms the scalars and the ticket).
struct Krylov {
  using Vec = double*;
  using CVec = const double*;
  Handle& h;
  int64_t n;
  DevBuf<double> partial, sc, hdev;        // partial sums; device scalars; coefficients of basis_update
  DevBuf<unsigned int> ticket;             // kr_dot_kernel's arrival counter (0 between launches)
  bool sr_partial_clean = false;
  int res = 0, op = 0, work_[3] = {0, 0, 0};     // Handle::kr_ws slots of the residual, the operand of A and the work vectors
  explicit Krylov(Handle& hh) : h(hh), n(hh.lev[0].len()) {
    if (hh.lev[0].n != hh.lev[0].ncols) throw Err("Krylov solvers need a square level-0 matrix (single rank)");
    partial.alloc((size_t)KR_BLOCKS * 64);
    sc.alloc(64);
    ticket.alloc(1);
    HIPCHK(hipMemsetAsync(sc.p, 0, 64 * sizeof(double), h.stream));
    HIPCHK(hipMemsetAsync(ticket.p, 0, sizeof(unsigned int), h.stream));
  }
  int nb() const { return (int)std::max<int64_t>(1, std::min<int64_t>(KR_BLOCKS, (n + BLOCK - 1) / BLOCK)); }
  int grid() const { return Handle::grid_for(n); }
  // work vectors live in the handle (grow-only) and keep their addresses from solve to solve: the cycle's graph is keyed on the
  // (right-hand side, result) pointers, so a solver that allocated per call paid a fresh capture + instantiation -- and the
  // hipMalloc / hipFree of its vectors (GMRES(30) at cfg 2: 2.6 GB) -- on every solve
  double* ws(int s, size_t count) {
    DevBuf<double>& b = h.kr_ws[s];
    if (b.n < count) b.alloc(count);
    return b.p;
  }
  // Handle::kr_ws slots by role: 0 / 1 / 2 serve CG (which feeds s = slot 2 to A), 0 .. 4 the single-reduction form (which feeds
  // u = slot 1), 5 / 1 / 2 GMRES (basis, w, t)
  void begin(Form f, int restart) {
    int first = 0, last = 2;                 // the slots of n entries this form uses
    if (f == Form::CG) { res = 0; work_[0] = 1; op = 2; }
    else if (f == Form::CG_SR) { res = 0; op = 1; work_[0] = 2; work_[1] = 3; work_[2] = 4; last = 4; }
    else {
      // (the basis lives in HBM: (restart + 1) vectors; multi_dot handles up to 48 of them per pass)
      if (restart > 40) throw Err("amgx_gmres: restart lengths above 40 are not supported (got " + std::to_string(restart) + ")");
      ws(5, (size_t)(std::max(1, restart) + 1) * n);
      work_[0] = 1; work_[1] = 2; first = 1;
      res = op = work_[2] = 5;               // GMRES has no residual / operand / third work vector: a use would name the basis, never an unsized slot
    }
    for (int s = first; s <= last; ++s) ws(s, n);
    if (f == Form::GMRES) hdev.alloc(64);
  }
  Vec residual_vec() { return h.kr_ws[res].p; }
  Vec operand() { return h.kr_ws[op].p; }
  Vec work(int k) { return h.kr_ws[work_[k]].p; }
  Vec basis(int j) { return h.kr_ws[5].p + (size_t)j * n; }

  void residual(CVec x, CVec b, Vec r) { h.residual(h.lev[0].A, x, b, r); }
  void mult(CVec v, Vec y) { h.mult(h.lev[0].A, v, y); }
  void precond(CVec r, Vec z, bool use_pre) {
    if (use_pre) h.run_cycle(z, r, true);
    else h.copy(z, r, n);
  }

  void dot(CVec a, CVec b, int s) { launch(kr_dot_kernel, nb(), BLOCK, 0, h.stream, n, a, b, partial.p, ticket.p, sc.p + s); }
  void multi_dot(int m, CVec w) {
    if (m > 48) throw Err("multi_dot: too many vectors");
    launch(kr_multi_dot_partial_kernel, nb(), BLOCK, 0, h.stream, n, m, basis(0), n, w, partial.p);
    launch(kr_dot_final_kernel, m, BLOCK, 0, h.stream, nb(), partial.p, sc.p);
  }
  void sr_reduce(CVec r, CVec u, CVec w) {
    if (!sr_partial_clean) {                 // (slots a short vector never writes)
      HIPCHK(hipMemsetAsync(partial.p, 0, (size_t)2 * KR_BLOCKS * sizeof(double), h.stream));
      sr_partial_clean = true;
    }
    launch(kr_dot2_partial_kernel, nb(), BLOCK, 0, h.stream, n, r, u, w, partial.p);
    launch(kr_sr_reduce_kernel, 2, BLOCK, 0, h.stream, 1, partial.p, sc.p);
    launch(kr_sr_scalars_kernel, 1, 1, 0, h.stream, sc.p);
  }
  double read(int s) {
    double v = 0.0;
    read(s, 1, &v);
    return v;
  }
  void read(int s0, int m, double* out) {
    HIPCHK(hipMemcpyAsync(out, sc.p + s0, m * sizeof(double), hipMemcpyDeviceToHost, h.stream));
    HIPCHK(hipStreamSynchronize(h.stream));
  }
  void write(int s, double v) { HIPCHK(hipMemcpyAsync(sc.p + s, &v, sizeof(double), hipMemcpyHostToDevice, h.stream)); }

  void copy(Vec dst, CVec src) { h.copy(dst, src, n); }
  void zero(Vec a, Vec b) { h.zero(a, n); h.zero(b, n); }
  void scale(double alpha, CVec x, Vec y) { launch(kr_scale_kernel, grid(), BLOCK, 0, h.stream, n, alpha, x, y, 0); }
  void cg_update(int num, int den, CVec s, CVec q, Vec x, Vec d) { launch(kr_cg_update_kernel, grid(), BLOCK, 0, h.stream, n, sc.p, num, den, s, q, x, d); }
  void xpby(int num, int den, CVec w, Vec s) { launch(kr_xpby_kernel, grid(), BLOCK, 0, h.stream, n, sc.p, num, den, w, s); }
  void sr_update(CVec u, CVec w, Vec p, Vec s, Vec x, Vec r) { launch(kr_sr_update_kernel, grid(), BLOCK, 0, h.stream, n, sc.p, u, w, p, s, x, r); }
  void basis_update(int m, const double* c, double sign, Vec w) {
    HIPCHK(hipMemcpyAsync(hdev.p, c, m * sizeof(double), hipMemcpyHostToDevice, h.stream));
    launch(kr_multi_axpy_kernel, grid(), BLOCK, 0, h.stream, n, m, basis(0), n, hdev.p, sign, w);
    HIPCHK(hipStreamSynchronize(h.stream));
  }
};

}  // namespace amgx

extern "C" {

int amgx_pcg(amgx_handle hh, const double* b, double* x, double tol, int maxit, int use_precond, int flags, double* errs, int32_t* iters) {
  return guard(hh, [&](amgx::Handle& h) {
    if (!b || !x || maxit < 0) throw amgx::Err("amgx_pcg: bad arguments");
    const int64_t n = h.lev[0].len();
    Staged st(h, flags);
    const double* db = st.in(0, b, n, 0);
    double* dx = st.inout(1, x, n, true, 0);
    if (use_precond && (db == h.lev[0].x.p || dx == h.lev[0].x.p)) throw amgx::Err("amgx_pcg: vectors alias the handle's work vectors");
    amgx::Krylov K(h);
    const int it = ((flags & AMGX_PCG_SINGLE_REDUCTION) && use_precond) ? amgx::pcg_sr(K, db, dx, tol, maxit, errs) : amgx::pcg(K, db, dx, tol, maxit, use_precond != 0, errs);
    if (iters) *iters = it;
    st.out(1, x, n, 0);
    st.finish();
  });
}

int amgx_gmres(amgx_handle hh, const double* b, double* x, double tol, int maxit, int restart, int use_precond, int flags, double* errs,
               int32_t* iters) {
  return guard(hh, [&](amgx::Handle& h) {
    if (!b || !x || maxit < 0 || restart < 1) throw amgx::Err("amgx_gmres: bad arguments");
    const int64_t n = h.lev[0].len();
    Staged st(h, flags);
    const double* db = st.in(0, b, n, 0);
    double* dx = st.inout(1, x, n, true, 0);
    if (use_precond && (db == h.lev[0].x.p || dx == h.lev[0].x.p)) throw amgx::Err("amgx_gmres: vectors alias the handle's work vectors");
    amgx::Krylov K(h);
    const int it = amgx::gmres(K, db, dx, tol, maxit, restart, use_precond != 0, errs);
    if (iters) *iters = it;
    st.out(1, x, n, 0);
    st.finish();
  });
}

}  // extern "C"
