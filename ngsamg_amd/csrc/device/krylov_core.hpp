// The Krylov recurrences, stated once: preconditioned CG, its single-reduction form and restarted GMRES over a *space* S that
// says where a vector lives and how a sum is formed.  krylov.hpp has the space of one handle (one pointer per vector, one-launch
// ticketed dot products), dist.hpp the space of a communicator (one pointer per local rank, halo exchange round the level-0
// product, partial + final launch and an all-reduce per sum).  Host-only: no HIP in here, so a plain C++17 compiler builds it
// (tests/test_krylov_core_cpu.py runs the three bodies over std::vector).
//
// What a space provides (a..z: S::Vec, a cheap handle; b of the solvers: S::CVec, its read-only form):
//   begin(form, restart)               work vectors of that recurrence exist from here on; rejects what the space cannot hold
//   residual_vec() operand() work(k) basis(j)     vectors by role: the residual the preconditioner reads in place, the vector
//                                      the operator reads in place, plain work vectors, column j of the GMRES basis
//   residual(x, b, r)  mult(v, y)      r = b - A x, y = A v (level 0)
//   precond(r, z, use_pre)             z = C r, or z = r
//   dot(a, b, slot)  read(slot)        <a, b> into a device scalar slot; its value on the host (synchronises)
//   multi_dot(m, w)  read(0, m, out)   slots 0 .. m-1 = <V_j, w> over the first m basis columns; their values on the host
//   write(slot, value)                 host value into a scalar slot
//   sr_reduce(r, u, w)                 slots SR_GNEW, SR_DELTA = <r, u>, <w, u>, then alpha / beta of the single-reduction step
//   copy(dst, src)  zero(a, b)  scale(alpha, x, y)      y = alpha x
//   cg_update(num, den, s, q, x, d)    alpha = slot[num] / slot[den] on the device: x += alpha s, d -= alpha q
//   xpby(num, den, w, s)               s = w + (slot[num] / slot[den]) s
//   sr_update(u, w, p, s, x, r)        p = u + beta p, s = w + beta s, x += alpha p, r -= alpha s
//   basis_update(m, c, sign, w)        w += sign * sum_j c[j] V_j with m host coefficients (uploads them; synchronises, so the
//                                      caller may overwrite c afterwards)
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <vector>

namespace amgx {

// scalar slots of the single-reduction recurrence
enum { SR_GOLD = 0, SR_GNEW = 1, SR_DELTA = 2, SR_ALPHA = 3, SR_BETA = 4, SR_FIRST = 5 };

enum class Form { CG, CG_SR, GMRES };        // the recurrence a space is asked to hold vectors for

// preconditioned CG (NGSolve CGSolver as the reference's drivers use it: err_k = sqrt(|<C r_k, r_k>|), stop at
// err_k <= tol * err_0; reference tests/h1/amg_utils.py:337-363).  x holds the initial guess.
template <class S>
int pcg(S& sp, typename S::CVec b, typename S::Vec x, double tol, int maxit, bool use_pre, double* errs) {
  sp.begin(Form::CG, 0);
  const typename S::Vec d = sp.residual_vec(), s = sp.operand(), w = sp.work(0);
  constexpr int SAS = 2;                                     // scalar slots: 0 / 1 = <w, d> of the last two iterations, 2 = <s, A s>
  sp.residual(x, b, d);                                      // d = b - A x
  sp.precond(d, w, use_pre);
  sp.copy(s, w);
  int cur = 1;
  sp.dot(w, d, cur);
  const double err0 = std::sqrt(std::fabs(sp.read(cur)));
  if (errs) errs[0] = err0;
  if (err0 == 0.0) return 0;
  int it = 0;
  for (it = 1; it <= maxit; ++it) {
    sp.mult(s, w);                                           // w = A s
    const int old = cur;
    cur = 1 - cur;
    sp.dot(s, w, SAS);
    sp.cg_update(old, SAS, s, w, x, d);                      // alpha = <w,d> / <s, A s>
    sp.precond(d, w, use_pre);
    sp.dot(w, d, cur);
    sp.xpby(cur, old, w, s);                                 // beta = <w,d>_new / <w,d>_old
    const double err = std::sqrt(std::fabs(sp.read(cur)));
    if (errs) errs[it] = err;
    if (err <= tol * err0) break;
  }
  if (it > maxit) it = maxit;
  return it;
}

// The same preconditioned CG with ONE reduction point per iteration (Chronopoulos / Gear): u = C r, w = A u, gamma = <r, u> and
// delta = <w, u> in one fused pass, alpha and beta from (gamma, delta) on the device, then p, s, x, r in one fused pass -- three
// launches per iteration beside the cycle and the level-0 product instead of five, and one device -> host scalar (over ranks: ONE
// all-reduce of (gamma, delta) instead of two of one scalar).  Mathematically the recurrence of pcg()
// (alpha_k = gamma_k / (delta_k - beta_k gamma_k / alpha_{k-1}) equals <C r, r> / <p, A p>); the rounding differs, histories
// agree to ~1e-6 (tests/test_gpu_krylov.py).  err_k = sqrt(|<C r_k, r_k>|) as in pcg().
template <class S>
int pcg_sr(S& sp, typename S::CVec b, typename S::Vec x, double tol, int maxit, double* errs) {
  sp.begin(Form::CG_SR, 0);
  const typename S::Vec r = sp.residual_vec(), u = sp.operand(), w = sp.work(0), p = sp.work(1), s = sp.work(2);
  sp.zero(p, s);
  sp.write(SR_FIRST, 1.0);
  sp.residual(x, b, r);                                      // r = b - A x
  sp.precond(r, u, true);
  sp.mult(u, w);
  sp.sr_reduce(r, u, w);
  const double err0 = std::sqrt(std::fabs(sp.read(SR_GOLD)));
  if (errs) errs[0] = err0;
  if (err0 == 0.0) return 0;
  int it = 0;
  for (it = 1; it <= maxit; ++it) {
    sp.sr_update(u, w, p, s, x, r);
    sp.precond(r, u, true);
    sp.mult(u, w);
    sp.sr_reduce(r, u, w);
    const double err = std::sqrt(std::fabs(sp.read(SR_GOLD)));
    if (errs) errs[it] = err;
    if (err <= tol * err0) break;
  }
  if (it > maxit) it = maxit;
  return it;
}

// host state of one GMRES(m) cycle: the rotated Hessenberg matrix H (upper triangular, row-major m columns), the Givens
// rotations (cs, sn), the rotated right-hand side g, the column being built (hcol) and the solution y of H y = g
struct Givens {
  int m;
  std::vector<double> H, cs, sn, g, hcol, y;
  explicit Givens(int mm) : m(mm), H((size_t)(mm + 1) * mm, 0.0), cs(mm), sn(mm), g(mm + 1), hcol(mm + 1), y(mm) {}
  void start(double beta) {
    std::fill(g.begin(), g.end(), 0.0);
    g[0] = beta;
  }
  // hcol[0 .. j+1] holds column j of the Hessenberg matrix: applies the previous rotations, forms rotation j, stores the column.
  // Returns the residual norm |g[j+1]| of the least-squares problem.
  double rotate(int j) {
    for (int i = 0; i < j; ++i) {                            // previous rotations
      const double a = cs[i] * hcol[i] + sn[i] * hcol[i + 1];
      hcol[i + 1] = -sn[i] * hcol[i] + cs[i] * hcol[i + 1];
      hcol[i] = a;
    }
    const double den = std::hypot(hcol[j], hcol[j + 1]);
    cs[j] = den > 0 ? hcol[j] / den : 1.0;
    sn[j] = den > 0 ? hcol[j + 1] / den : 0.0;
    hcol[j] = den;
    g[j + 1] = -sn[j] * g[j];
    g[j] = cs[j] * g[j];
    for (int i = 0; i <= j; ++i) H[(size_t)i * m + j] = hcol[i];
    return std::fabs(g[j + 1]);
  }
  // y = H^-1 g over the first k columns (upper triangular)
  const double* solve(int k) {
    for (int i = k - 1; i >= 0; --i) {
      double sacc = g[i];
      for (int q = i + 1; q < k; ++q) sacc -= H[(size_t)i * m + q] * y[q];
      const double piv = H[(size_t)i * m + i];
      // a zero pivot = the Krylov space stopped growing with a singular projected system (breakdown without convergence,
      // e.g. a singular operator): that direction gets no update instead of an inf / nan
      y[i] = piv != 0.0 ? sacc / piv : 0.0;
    }
    return y.data();
  }
};

// restarted GMRES(m), left-preconditioned: minimises |C (b - A x)|; classical Gram-Schmidt with one re-orthogonalisation
// pass (two fused passes over the basis instead of 2 j dependent dot / axpy pairs; the reference's driver is
// ngsolve.krylovspace.GMRes: one inner product at a time), Givens rotations on the host -- over ranks identically on every
// rank, all of them read the same reduced values.  err_k = |C r_k| (the recurrence value), stop at err_k <= tol * err_0.
// err0 < 0 marks the first restart cycle; with maxit = 0 nothing runs and errs[0] stays as the caller passed it.
template <class S>
int gmres(S& sp, typename S::CVec b, typename S::Vec x, double tol, int maxit, int restart, bool use_pre, double* errs) {
  sp.begin(Form::GMRES, restart);
  const int m = std::max(1, restart);
  const typename S::Vec w = sp.work(0), t = sp.work(1);
  Givens G(m);
  std::vector<double> hc2(m + 1);
  int it = 0;
  double err0 = -1.0;
  while (it < maxit) {
    sp.residual(x, b, t);                                    // t = b - A x
    sp.precond(t, sp.basis(0), use_pre);                     // v_0 = C t (not yet normalised)
    sp.dot(sp.basis(0), sp.basis(0), 0);
    const double beta = std::sqrt(sp.read(0));
    if (err0 < 0.0) { err0 = beta; if (errs) errs[0] = err0; }
    if (beta == 0.0 || beta <= tol * err0) break;
    sp.scale(1.0 / beta, sp.basis(0), sp.basis(0));
    G.start(beta);
    int j = 0;
    bool done = false;
    for (j = 0; j < m && it < maxit; ++j) {
      ++it;
      sp.mult(sp.basis(j), t);
      sp.precond(t, w, use_pre);                             // w = C A v_j
      std::fill(G.hcol.begin(), G.hcol.end(), 0.0);
      for (int pass = 0; pass < 2; ++pass) {
        sp.multi_dot(j + 1, w);
        sp.read(0, j + 1, hc2.data());
        sp.basis_update(j + 1, hc2.data(), -1.0, w);         // (synchronises: hc2 is reused by the next pass)
        for (int i = 0; i <= j; ++i) G.hcol[i] += hc2[i];
      }
      sp.dot(w, w, 0);
      const double hn = std::sqrt(sp.read(0));
      G.hcol[j + 1] = hn;
      if (hn > 0.0) sp.scale(1.0 / hn, w, sp.basis(j + 1));
      const double err = G.rotate(j);
      if (errs) errs[it] = err;
      if (err <= tol * err0 || hn == 0.0) { done = true; ++j; break; }
    }
    if (j > 0) sp.basis_update(j, G.solve(j), 1.0, x);       // x += V y
    if (done) break;
  }
  return it;
}

}  // namespace amgx
