// Multi-vector algebra on the handle's device and stream: amgx_mv_gram, amgx_mv_combine.
//
// This file is the host side; the kernels are in mv_kernels.hpp.  The work space (partial Gram matrices, the staged copies of
// host-pointer arguments, a small ring of coefficient matrices) is created by the first call and kept until amgx_destroy, like the
// multi-vector work space of multi.hpp.
#pragma once

namespace amgx {

struct MvState {
  DevBuf<double> partial, out;           // [MV_MAX^2][MV_BLOCKS] partial sums, [MV_MAX^2] sums
  DevBuf<double> stage[2];               // host-pointer calls: compact copies of the two multi-vectors
  // coefficient matrices of amgx_mv_combine travel through a ring: pinned host slot -> device slot on the stream, so that a call
  // with device vectors never waits for the GPU (a slot is reused only after the copy that read it has run)
  static constexpr int RING = 16;
  double* c_host = nullptr;              // RING x MV_MAX^2, pinned
  DevBuf<double> c_dev;
  hipEvent_t c_done[RING] = {};
  int c_next = 0;
  ~MvState() {
    for (auto& e : c_done) if (e) (void)hipEventDestroy(e);
    if (c_host) (void)hipHostFree(c_host);
  }
};
void mv_free(MvState* s) { delete s; }

struct Mv {
  Handle& h;
  MvState& st;
  explicit Mv(Handle& hh) : h(hh), st(state(hh)) {}
  static MvState& state(Handle& h) {
    if (!h.mv) h.mv = new MvState;
    return *h.mv;
  }
  static void fit(DevBuf<double>& b, int64_t n) { if ((int64_t)b.n < n) b.alloc((size_t)n); }

  // the launch shape of a Gram product: a function of (n, ka, kb, symmetric) alone
  static void gram_shape(int64_t n, int ka, int kb, bool sym, int* rc, int* nb) {
    *rc = mv_chunk_rows(sym ? ka : ka + kb);
    *nb = (int)std::max<int64_t>(1, std::min<int64_t>(MV_BLOCKS, (n + *rc - 1) / *rc));
  }

  // G (host, ka x kb row-major) = A^T B on device multi-vectors
  void gram(int64_t n, int ka, const double* A, int64_t lda, int kb, const double* B, int64_t ldb, bool il, bool sym, double* G) {
    if (n == 0) { std::fill(G, G + (size_t)ka * kb, 0.0); return; }
    if (!st.partial.p) { st.partial.alloc((size_t)MV_MAX * MV_MAX * MV_BLOCKS); st.out.alloc((size_t)MV_MAX * MV_MAX); }
    int rc, nb;
    gram_shape(n, ka, kb, sym, &rc, &nb);
    const int ta = (ka + 15) / 16, tb = (kb + 15) / 16, nc = sym ? ka : ka + kb;
    const size_t lds = sizeof(double) * std::max<size_t>((size_t)nc * (rc + MV_PAD), (size_t)WAVES_PER_BLOCK * ta * tb * 256);
    auto run = [&](auto TA, auto TB, auto SYM, auto IL) {
      launch(mv_gram_kernel<TA(), TB(), SYM(), IL()>, nb, BLOCK, lds, h.stream, n, ka, kb, A, lda, B, ldb, rc, st.partial.p);
    };
    auto by_il = [&](auto TA, auto TB, auto SYM) { if (il) run(TA, TB, SYM, std::true_type{}); else run(TA, TB, SYM, std::false_type{}); };
    auto by_sym = [&](auto TA, auto TB) { if (sym) by_il(TA, TB, std::true_type{}); else by_il(TA, TB, std::false_type{}); };
    auto by_tb = [&](auto TA) { if (tb == 1) by_sym(TA, Int<1>{}); else by_sym(TA, Int<2>{}); };
    if (ta == 1) by_tb(Int<1>{}); else by_tb(Int<2>{});
    launch(mv_gram_final_kernel, ka * kb, BLOCK, 0, h.stream, nb, kb, sym ? 1 : 0, st.partial.p, st.out.p);
    HIPCHK(hipMemcpyAsync(G, st.out.p, (size_t)ka * kb * sizeof(double), hipMemcpyDeviceToHost, h.stream));
    HIPCHK(hipStreamSynchronize(h.stream));
    if (sym)                                                   // the upper triangle, mirrored: symmetric bit for bit
      for (int i = 0; i < ka; ++i)
        for (int j = 0; j < i; ++j) G[i * kb + j] = G[j * kb + i];
  }

  // Y = beta Y + X c on device multi-vectors; c: host, kx x ky row-major
  void combine(int64_t n, int kx, const double* X, int64_t ldx, const double* c, int ky, double beta, double* Y, int64_t ldy, bool il) {
    if (n == 0) return;
    const int kyt = ky <= 1 ? 1 : ky <= 2 ? 2 : ky <= 4 ? 4 : ky <= 8 ? 8 : ky <= 16 ? 16 : ky <= 24 ? 24 : 32;
    constexpr size_t SLOT = (size_t)MV_MAX * MV_MAX;
    if (!st.c_host) {
      HIPCHK(hipHostMalloc((void**)&st.c_host, MvState::RING * SLOT * sizeof(double), hipHostMallocDefault));
      st.c_dev.alloc(MvState::RING * SLOT);
      for (auto& e : st.c_done) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    const int slot = st.c_next;
    st.c_next = (slot + 1) % MvState::RING;
    HIPCHK(hipEventSynchronize(st.c_done[slot]));              // (an event that was never recorded is complete)
    double* ch = st.c_host + slot * SLOT;
    double* cd = st.c_dev.p + slot * SLOT;
    for (int i = 0; i < kx; ++i)
      for (int j = 0; j < kyt; ++j) ch[i * kyt + j] = j < ky ? c[i * ky + j] : 0.0;
    HIPCHK(hipMemcpyAsync(cd, ch, (size_t)kx * kyt * sizeof(double), hipMemcpyHostToDevice, h.stream));
    HIPCHK(hipEventRecord(st.c_done[slot], h.stream));
    const int64_t xrs = il ? kx : 1, xcs = il ? 1 : ldx, yrs = il ? ky : 1, ycs = il ? 1 : ldy;
    const int64_t grid = (n + BLOCK - 1) / BLOCK;
    if (grid > INT_MAX) throw Err("amgx_mv_combine: n is too large for one launch");
    auto run = [&](auto KYT) { launch(mv_combine_kernel<KYT()>, (int)grid, BLOCK, 0, h.stream, n, kx, ky, X, xrs, xcs, cd, beta, Y, yrs, ycs); };
    if (!dispatch<1, 2, 4, 8, 16, 24, 32>(kyt, run)) throw Err("amgx_mv_combine: no kernel for this width");
  }

  // host-pointer arguments: a compact copy (column-major: ld = n) on the device
  const double* stage_in(int which, const double* p, int64_t n, int k, bool il, int64_t ld, bool load) {
    DevBuf<double>& buf = st.stage[which];
    fit(buf, n * k);
    if (load && n > 0) {
      if (il || ld == n) HIPCHK(hipMemcpyAsync(buf.p, p, (size_t)n * k * sizeof(double), hipMemcpyHostToDevice, h.stream));
      else HIPCHK(hipMemcpy2DAsync(buf.p, (size_t)n * sizeof(double), p, (size_t)ld * sizeof(double), (size_t)n * sizeof(double), k, hipMemcpyHostToDevice, h.stream));
    }
    return buf.p;
  }
  void stage_out(int which, double* p, int64_t n, int k, bool il, int64_t ld) {
    if (n == 0) return;
    const DevBuf<double>& buf = st.stage[which];
    if (il || ld == n) HIPCHK(hipMemcpyAsync(p, buf.p, (size_t)n * k * sizeof(double), hipMemcpyDeviceToHost, h.stream));
    else HIPCHK(hipMemcpy2DAsync(p, (size_t)ld * sizeof(double), buf.p, (size_t)n * sizeof(double), (size_t)n * sizeof(double), k, hipMemcpyDeviceToHost, h.stream));
    HIPCHK(hipStreamSynchronize(h.stream));
  }
};

inline void mv_check(const std::string& f, int64_t n, int k, const void* p, int64_t ld, bool il, const char* name) {
  if (n < 0) throw Err(f + ": n must not be negative (got " + std::to_string(n) + ")");
  if (k < 1 || k > MV_MAX) throw Err(f + ": " + name + " has " + std::to_string(k) + " columns, need 1 .. AMGX_MV_MAX = " + std::to_string(MV_MAX));
  if (n > 0 && !p) throw Err(f + ": " + name + " is a null pointer");
  if (!il && ld < n) throw Err(f + ": leading dimension of " + name + " (" + std::to_string(ld) + ") is below n = " + std::to_string(n));
}

}  // namespace amgx

extern "C" {

int amgx_mv_gram(amgx_handle hh, int64_t n, int ka, const double* A, int64_t lda, int kb, const double* B, int64_t ldb, double* G, int flags) {
  return guard(hh, [&](amgx::Handle& h) {
    const std::string fn = "amgx_mv_gram";
    const bool il = flags & AMGX_MULTI_INTERLEAVED, host = !(flags & AMGX_DEVICE_PTR);
    amgx::mv_check(fn, n, ka, A, lda, il, "A");
    amgx::mv_check(fn, n, kb, B, ldb, il, "B");
    if (!G) throw amgx::Err(fn + ": G is a null pointer");
    const bool sym = A == B && ka == kb && (il || lda == ldb);
    amgx::Mv M(h);
    const double *dA = A, *dB = B;
    int64_t la = lda, lb = ldb;
    if (host) {
      dA = M.stage_in(0, A, n, ka, il, lda, true);
      dB = sym ? dA : M.stage_in(1, B, n, kb, il, ldb, true);
      la = lb = n;
    }
    M.gram(n, ka, dA, la, kb, dB, lb, il, sym, G);
  });
}

int amgx_mv_gram_plan(amgx_handle hh, int64_t n, int ka, int kb, int symmetric, int32_t* chunk_rows, int32_t* n_blocks) {
  return guard(hh, [&](amgx::Handle&) {
    const std::string fn = "amgx_mv_gram_plan";
    if (n < 0) throw amgx::Err(fn + ": n must not be negative");
    if (ka < 1 || ka > amgx::MV_MAX || kb < 1 || kb > amgx::MV_MAX || (symmetric && ka != kb))
      throw amgx::Err(fn + ": need 1 <= ka, kb <= AMGX_MV_MAX = " + std::to_string(amgx::MV_MAX) + " (ka == kb when symmetric)");
    int rc, nb;
    amgx::Mv::gram_shape(n, ka, kb, symmetric != 0, &rc, &nb);
    if (chunk_rows) *chunk_rows = rc;
    if (n_blocks) *n_blocks = n > 0 ? nb : 0;
  });
}

int amgx_mv_combine(amgx_handle hh, int64_t n, int kx, const double* X, int64_t ldx, const double* c, int ky, double beta, double* Y, int64_t ldy,
                    int flags) {
  return guard(hh, [&](amgx::Handle& h) {
    const std::string fn = "amgx_mv_combine";
    const bool il = flags & AMGX_MULTI_INTERLEAVED, host = !(flags & AMGX_DEVICE_PTR);
    amgx::mv_check(fn, n, kx, X, ldx, il, "X");
    amgx::mv_check(fn, n, ky, Y, ldy, il, "Y");
    if (!c) throw amgx::Err(fn + ": c is a null pointer");
    if (n > 0 && X == Y) throw amgx::Err(fn + ": Y must not be one of the X arrays (the same base pointer was passed)");
    if (n == 0) return;
    amgx::Mv M(h);
    if (!host) { M.combine(n, kx, X, ldx, c, ky, beta, Y, ldy, il); return; }
    const double* dX = M.stage_in(0, X, n, kx, il, ldx, true);
    double* dY = const_cast<double*>(M.stage_in(1, Y, n, ky, il, ldy, beta != 0.0));
    M.combine(n, kx, dX, n, c, ky, beta, dY, n, il);
    M.stage_out(1, Y, n, ky, il, ldy);
  });
}

}  // extern "C"
