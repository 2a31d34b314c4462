// The Chebyshev smoother's recurrence, stated once: which pass of one smooth of degree k reads and writes which vector.
// Handle::cheb_smooth (amgx.hip) runs it with cheb_first / cheb_step, Multi::cycle_v_multi (multi.hpp) with the diagonal and the
// EP_CHEB product on interleaved vectors.  Host-only: no HIP in here, so a plain C++17 compiler builds it
// (tests/test_cheb_schedule_cpu.py runs it over std::vector).
//
//   d_1 = c0 Dinv (b - A x_0),  d_j = c1[j] d_{j-1} + c2[j] Dinv (b - A x_{j-1}),  x_j = x_{j-1} + d_j        (j = 2 .. k)
//
// The callables:
//   first(v, xin, xout, dout, c0)            xout = (xin ? xin : 0) + c0 Dinv v; dout (optional) = the update.  No product.
//   step(xin, xout, c1, c2, d_old, d_new)    xout = xin + d_new, d_new = c1 d_old + c2 Dinv (b - A xin), out of place.
//                                            d_old == nullptr: d_old is xin itself; d_new == nullptr: not stored.
//   exchange(v)  (optional; default: nothing)  rank-partitioned levels: a product step reads its input on [owned | ghost] and
//                                            writes owned rows, so the owner -> ghost exchange of the iterate v precedes every
//                                            product step whose input ghosts are not known.  They are known in one case only: the
//                                            step after first() from zero when the caller's first() covers the ghost rows too (b
//                                            and Dinv are at hand there: `ghosts_after_first`).  d lives on owned rows.
#pragma once

namespace amgx {

// what the caller knows on entry (the flag contract of base_smooth): x = 0; v holds the residual b - A x of the iterate; neither
enum class ChebEntry { ZERO, RES_UPDATED, ITERATE };

// product passes of one smooth: step 1 needs none when x = 0 (then b is the residual) or when the residual is at hand
inline int cheb_passes(int k, ChebEntry e) { return k - 1 + (e == ChebEntry::ITERATE ? 1 : 0); }

// where a caller that can choose puts the iterate ahead of `passes` out-of-place passes between x and tmp, so that the last one
// lands in x (post_smooth and the multi-vector up pass: t = x + P x_c, passes = k)
template <class T>
T* cheb_place(int passes, T* x, T* tmp) { return (passes & 1) ? tmp : x; }

struct ChebNoExchange { void operator()(const double*) const {} };

// exchanges of one smooth on a rank-partitioned level: one per product pass, less the one that first() from zero saves
inline int cheb_exchanges(int k, ChebEntry e, bool ghosts_after_first) {
  return cheb_passes(k, e) - ((ghosts_after_first && e == ChebEntry::ZERO && k > 1) ? 1 : 0);
}

// One smooth of degree k.  The iterate lives in `src` (x or tmp; ignored with ZERO); v is what step 1 reads without a product (b
// with ZERO, the residual with RES_UPDATED; ignored with ITERATE).  The steps ping-pong between x and tmp; d holds the update of
// the previous step whenever another step follows -- except after the first step from zero, where the update is the iterate
// itself.  Returns where the result lies: x, unless `src` left an odd number of passes (then the caller copies).
template <class First, class Step, class Exchange = ChebNoExchange>
double* cheb_schedule(int k, double c0, const double* c1, const double* c2, ChebEntry entry, const double* v, const double* src,
                      double* x, double* tmp, double* d, First&& first, Step&& step, Exchange&& exchange = Exchange(),
                      bool ghosts_after_first = false) {
  double* cur;
  bool ghosts_known = false;              // the ghost entries of the iterate are current (rank-partitioned levels)
  const double* dcur = d;                 // where d of the previous step lives (nullptr: in the iterate itself)
  if (entry != ChebEntry::ITERATE) {
    const bool zero = entry == ChebEntry::ZERO;
    cur = cheb_place(k - 1, x, tmp);
    first(v, zero ? nullptr : src, cur, (!zero && k > 1) ? d : nullptr, c0);
    if (zero) dcur = nullptr;
    ghosts_known = zero && ghosts_after_first;
  } else {                                // step 1 as a product step: (c1, c2) = (0, c0) on d_old = the iterate
    cur = src == x ? tmp : x;
    exchange(src);
    step(src, cur, 0.0, c0, nullptr, k > 1 ? d : nullptr);
  }
  for (int j = 2; j <= k; ++j) {
    double* nxt = cur == x ? tmp : x;
    if (!ghosts_known) exchange(cur);
    ghosts_known = false;
    step(cur, nxt, c1[j], c2[j], dcur, j < k ? d : nullptr);
    dcur = d;
    cur = nxt;
  }
  return cur;
}

}  // namespace amgx
