"""The exchange points of ngsamg_amd/csrc/device/cheb_schedule.hpp (the optional `exchange` callable) on emulated rank-partitioned
vectors, compiled by a plain C++17 host compiler.

A 1-D Laplacian-like matrix (n = 13, varying diagonal) is cut into 2 and into 3 ranks of unequal size.  Every rank keeps its
owned rows over [owned | ghost] columns, the iterate buffers x and tmp in that layout, d and the residual on owned rows -- the
layout of the device drivers (DistCycle::cheb_smooth), which walk the schedule once for all ranks with tokens for the vectors; so
does this program.  A product step reads its input on [owned | ghost] and writes owned rows.  Ghost entries of the iterate change
only inside the exchange callable and are set to NaN after every pass, so a step that reads a ghost the schedule did not
exchange turns its rows into NaN.  The one other writer is first() from zero with `ghosts_after_first`: it forms x_1 on the ghost
rows too, from the right-hand side and Dinv there (what the overlapped driver does with the exchanged b).

Degrees 1 .. 4, the entries ZERO / RES_UPDATED / ITERATE, the iterate in x and in tmp, with and without ghosts_after_first.
Checked: the owned entries equal the serial schedule on the global vectors to 1e-14 relative with no NaN; the number of exchanges
is at most the number of product passes and equals cheb_exchanges()."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include "cheb_schedule.hpp"
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

using amgx::ChebEntry;
using Vec = std::vector<double>;
constexpr int N = 13;
static double A[N][N], dinv[N], bg[N], x0g[N];

struct Rank {
  int lo, hi;                       // owned global rows [lo, hi)
  std::vector<int> ghost;           // global index of every ghost entry
  int n() const { return hi - lo; }
  int ext() const { return n() + (int)ghost.size(); }
  int glob(int j) const { return j < n() ? lo + j : ghost[j - n()]; }
  int loc(int g) const {            // local column of global g (-1: not stored)
    if (g >= lo && g < hi) return g - lo;
    for (size_t q = 0; q < ghost.size(); ++q) if (ghost[q] == g) return n() + (int)q;
    return -1;
  }
  Vec x, tmp, d, res, b;            // x, tmp, b: [owned | ghost]; d, res: owned
};

int main() {
  for (int i = 0; i < N; ++i) {
    A[i][i] = 2.5 + 0.125 * i;
    if (i + 1 < N) A[i][i + 1] = A[i + 1][i] = -1.0 - 0.0625 * i;
    dinv[i] = 1.0 / A[i][i];
    bg[i] = 1.0 + 0.37 * i - 0.05 * i * i;
    x0g[i] = 0.3 - 0.11 * i + 0.02 * i * i;
  }
  const double c0 = 0.61, nan = std::numeric_limits<double>::quiet_NaN();
  double c1[9], c2[9];
  for (int j = 0; j < 9; ++j) { c1[j] = 0.08 + 0.031 * j; c2[j] = 0.52 + 0.023 * j; }
  const std::vector<std::vector<int>> cuts = {{0, 5, N}, {0, 3, 9, N}};
  const ChebEntry entries[] = {ChebEntry::ZERO, ChebEntry::RES_UPDATED, ChebEntry::ITERATE};
  int bad = 0, cases = 0;
  for (const auto& cut : cuts) for (int k = 1; k <= 4; ++k) for (ChebEntry entry : entries) for (int src_in_tmp = 0; src_in_tmp < 2; ++src_in_tmp)
  for (int gaf = 0; gaf < 2; ++gaf) {
    ++cases;
    const int R = (int)cut.size() - 1;
    auto fail = [&](const char* what) { std::printf("R=%d k=%d entry=%d src_in_tmp=%d gaf=%d: %s\n", R, k, (int)entry, src_in_tmp, gaf, what); ++bad; };
    const bool zero = entry == ChebEntry::ZERO;
    // ---- the serial schedule on the global vectors
    Vec gx(N, 0.0), gt(N, 0.0), gd(N, 0.0), gres(N, 0.0);
    double* const gsrc = src_in_tmp ? gt.data() : gx.data();
    if (!zero) for (int i = 0; i < N; ++i) gsrc[i] = x0g[i];
    for (int i = 0; i < N; ++i) { double ax = 0.0; for (int j = 0; j < N; ++j) ax += A[i][j] * x0g[j]; gres[i] = bg[i] - ax; }
    auto sfirst = [&](const double* v, const double* xin, double* xout, double* dout, double cc) {
      for (int i = 0; i < N; ++i) { const double u = cc * (dinv[i] * v[i]); xout[i] = xin ? xin[i] + u : u; if (dout) dout[i] = u; }
    };
    auto sstep = [&](const double* xin, double* xout, double s1, double s2, const double* d_old, double* d_new) {
      Vec out(N);
      for (int i = 0; i < N; ++i) {
        double ax = 0.0;
        for (int j = 0; j < N; ++j) ax += A[i][j] * xin[j];
        const double dn = s1 * (d_old ? d_old[i] : xin[i]) + s2 * (dinv[i] * (bg[i] - ax));
        out[i] = xin[i] + dn;
        if (d_new) d_new[i] = dn;
      }
      for (int i = 0; i < N; ++i) xout[i] = out[i];
    };
    const double* gend = amgx::cheb_schedule(k, c0, c1, c2, entry, entry == ChebEntry::RES_UPDATED ? gres.data() : bg, gsrc, gx.data(), gt.data(),
                                             gd.data(), sfirst, sstep);
    // ---- the ranks
    std::vector<Rank> rk(R);
    for (int r = 0; r < R; ++r) {
      Rank& q = rk[r];
      q.lo = cut[r]; q.hi = cut[r + 1];
      if (r > 0) q.ghost.push_back(q.lo - 1);
      if (r + 1 < R) q.ghost.push_back(q.hi);
      q.x.assign(q.ext(), nan); q.tmp.assign(q.ext(), nan); q.b.assign(q.ext(), nan);
      q.d.assign(q.n(), nan); q.res.assign(q.n(), nan);
      for (int j = 0; j < q.ext(); ++j) q.b[j] = bg[q.glob(j)];          // (the right-hand side after its own exchange)
      for (int j = 0; j < q.n(); ++j) q.res[j] = gres[q.lo + j];
      if (!zero) for (int j = 0; j < q.n(); ++j) (src_in_tmp ? q.tmp : q.x)[j] = x0g[q.lo + j];
    }
    double tx = 0, tt = 0, td = 0, tv = 0;                               // the schedule's vectors as tokens
    (void)tx; (void)tt; (void)td; (void)tv;
    auto it_of = [&](Rank& q, const double* p) -> Vec& { return p == &tx ? q.x : q.tmp; };
    auto poison = [&]() { for (Rank& q : rk) for (int j = q.n(); j < q.ext(); ++j) q.x[j] = q.tmp[j] = nan; };
    int n_exchange = 0, n_step = 0;
    auto first = [&](const double* v, const double* xin, double* xout, double* dout, double cc) {
      if (v != &tv) fail("first(): v");
      for (Rank& q : rk) {
        const Vec& vv = entry == ChebEntry::RES_UPDATED ? q.res : q.b;
        const int rows = (zero && gaf) ? q.ext() : q.n();               // from zero the ghost rows can be formed locally
        Vec& out = it_of(q, xout);
        for (int j = 0; j < rows; ++j) {
          const double u = cc * (dinv[q.glob(j)] * vv[j]);
          out[j] = xin ? it_of(q, xin)[j] + u : u;
          if (dout && j < q.n()) q.d[j] = u;
        }
      }
      if (!(zero && gaf)) poison();
    };
    auto exchange = [&](const double* v) {
      ++n_exchange;
      if (v != &tx && v != &tt) fail("exchange(): not an iterate buffer");
      for (Rank& q : rk)
        for (int j = q.n(); j < q.ext(); ++j) {
          const int g = q.glob(j);
          for (Rank& o : rk) if (g >= o.lo && g < o.hi) it_of(q, v)[j] = it_of(o, v)[g - o.lo];
        }
    };
    auto step = [&](const double* xin, double* xout, double s1, double s2, const double* d_old, double* d_new) {
      ++n_step;
      if (d_old && d_old != &td) fail("step(): d_old");
      if (d_new && d_new != &td) fail("step(): d_new");
      for (Rank& q : rk) {
        const Vec& in = it_of(q, xin);
        Vec out(q.n());
        for (int j = 0; j < q.n(); ++j) {
          double ax = 0.0;
          for (int g = 0; g < N; ++g) if (A[q.lo + j][g] != 0.0) { const int cidx = q.loc(g); if (cidx < 0) fail("a row reads a column the rank does not store"); else ax += A[q.lo + j][g] * in[cidx]; }
          const double dn = s1 * (d_old ? q.d[j] : in[j]) + s2 * (dinv[q.lo + j] * (q.b[j] - ax));
          out[j] = in[j] + dn;
          if (d_new) q.d[j] = dn;
        }
        Vec& o = it_of(q, xout);
        for (int j = 0; j < q.n(); ++j) o[j] = out[j];
      }
      poison();
    };
    const double* end = amgx::cheb_schedule(k, c0, c1, c2, entry, &tv, src_in_tmp ? &tt : &tx, &tx, &tt, &td, first, step, exchange, gaf != 0);
    if ((end == &tt) != (gend == gt.data())) fail("the result lies in another buffer than the serial schedule's");
    const int passes = amgx::cheb_passes(k, entry);
    if (n_step != passes) fail("product steps != cheb_passes");
    if (n_exchange > passes) fail("more exchanges than product passes");
    if (n_exchange != amgx::cheb_exchanges(k, entry, gaf != 0)) fail("exchanges != cheb_exchanges");
    for (Rank& q : rk) {
      const Vec& got = it_of(q, end);
      for (int j = 0; j < q.n(); ++j) {
        const double ref = gend[q.lo + j];
        if (std::isnan(got[j])) { fail("NaN in an owned entry: a pass read a ghost that was not exchanged"); break; }
        if (!(std::fabs(got[j] - ref) <= 1e-14 * std::fabs(ref))) { fail("x differs from the serial schedule"); break; }
      }
    }
  }
  // the default callable: nothing is exchanged, the serial callers compile unchanged (checked above: gend)
  if (amgx::cheb_exchanges(1, ChebEntry::ZERO, true) != 0 || amgx::cheb_exchanges(2, ChebEntry::ZERO, true) != 0 ||
      amgx::cheb_exchanges(3, ChebEntry::ZERO, true) != 1 || amgx::cheb_exchanges(3, ChebEntry::ZERO, false) != 2 ||
      amgx::cheb_exchanges(3, ChebEntry::ITERATE, true) != 3) { std::printf("cheb_exchanges\n"); ++bad; }
  std::printf("cases=%d bad=%d\n", cases, bad);
  return bad ? 1 : 0;
}
"""


def test_cheb_schedule_exchange_points_on_emulated_ranks(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to compile cheb_schedule.hpp")
    src = tmp_path / "cheb_schedule_dist_check.cpp"
    exe = tmp_path / "cheb_schedule_dist_check"
    src.write_text(PROGRAM)
    inc = os.path.join(ROOT, "ngsamg_amd", "csrc", "device")
    cc = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", inc, "-o", str(exe), str(src)],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip().endswith("cases=96 bad=0"), run.stdout
