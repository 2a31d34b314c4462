"""ngsamg_amd/csrc/device/cheb_schedule.hpp (the Chebyshev smoother's recurrence as a schedule of first / step calls) compiled by a
plain C++17 host compiler and run over std::vector on a small dense SPD matrix (n = 7: tridiagonal plus one far entry).

Degrees 1 .. 4 and 8, the three entry states, the iterate in x and in tmp.  Checked: the result is in x (after the copy the schedule
asks for, if any) and equals the recurrence written out literally to 1e-14 relative (same arithmetic in the same order: the bound
only allows for compiler contraction); d_old / d_new follow the stated rule; the number of product steps is cheb_passes; no copy
whenever the iterate is placed as post_smooth places it (cheb_place).  Vectors that a pass must not read hold NaN."""
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
constexpr int N = 7;

static double A[N][N], dinv[N];
static Vec matvec(const double* x) {
  Vec y(N, 0.0);
  for (int i = 0; i < N; ++i)
    for (int j = 0; j < N; ++j) y[i] += A[i][j] * x[j];
  return y;
}

int main() {
  for (int i = 0; i < N; ++i) {
    A[i][i] = 4.0 + 0.25 * i;
    if (i + 1 < N) A[i][i + 1] = A[i + 1][i] = -1.0 - 0.125 * i;
    dinv[i] = 1.0 / A[i][i];
  }
  A[0][5] = A[5][0] = -0.5;
  Vec b(N), x0(N);
  for (int i = 0; i < N; ++i) { b[i] = 1.0 + 0.37 * i - 0.05 * i * i; x0[i] = 0.3 - 0.11 * i + 0.02 * i * i; }
  const double c0 = 0.61;
  double c1[9], c2[9];
  for (int j = 0; j < 9; ++j) { c1[j] = 0.08 + 0.031 * j; c2[j] = 0.52 + 0.023 * j; }
  const double nan = std::numeric_limits<double>::quiet_NaN();
  int bad = 0, cases = 0;
  const int degrees[] = {1, 2, 3, 4, 8};
  const ChebEntry entries[] = {ChebEntry::ZERO, ChebEntry::RES_UPDATED, ChebEntry::ITERATE};
  for (int k : degrees) for (ChebEntry entry : entries) for (int src_in_tmp = 0; src_in_tmp < 2; ++src_in_tmp) {
    ++cases;
    const int e = (int)entry;
    auto fail = [&](const char* what) { std::printf("k=%d entry=%d src_in_tmp=%d: %s\n", k, e, src_in_tmp, what); ++bad; };
    const bool zero = entry == ChebEntry::ZERO;
    // ---- the recurrence, literally
    Vec xr = zero ? Vec(N, 0.0) : x0, dr(N);
    {
      const Vec ax = matvec(xr.data());
      for (int i = 0; i < N; ++i) {
        const double r = zero ? b[i] : b[i] - ax[i];       // (from zero the right-hand side is the residual)
        dr[i] = c0 * (dinv[i] * r);
        xr[i] = zero ? dr[i] : xr[i] + dr[i];
      }
    }
    for (int j = 2; j <= k; ++j) {
      const Vec ax = matvec(xr.data());
      for (int i = 0; i < N; ++i) {
        dr[i] = c1[j] * dr[i] + c2[j] * (dinv[i] * (b[i] - ax[i]));
        xr[i] = xr[i] + dr[i];
      }
    }
    // ---- the schedule
    Vec x(N, nan), tmp(N, nan), d(N, nan), res(N, nan);
    double* const src = src_in_tmp ? tmp.data() : x.data();
    if (!zero) for (int i = 0; i < N; ++i) src[i] = x0[i];
    if (entry == ChebEntry::RES_UPDATED) { const Vec ax = matvec(x0.data()); for (int i = 0; i < N; ++i) res[i] = b[i] - ax[i]; }
    const double* const v = entry == ChebEntry::RES_UPDATED ? res.data() : b.data();
    int n_first = 0, n_step = 0;
    auto in_pair = [&](const double* p) { return p == x.data() || p == tmp.data(); };
    auto first = [&](const double* vv, const double* xin, double* xout, double* dout, double cc) {
      ++n_first;
      if (n_step) fail("first() after a product step");
      if (vv != v || cc != c0) fail("first(): v or c0");
      if (xin != (zero ? nullptr : src)) fail("first(): xin");
      if (!in_pair(xout)) fail("first(): xout is neither x nor tmp");
      if (dout != ((!zero && k > 1) ? d.data() : nullptr)) fail("first(): d is stored exactly when the iterate is not zero and a step follows");
      for (int i = 0; i < N; ++i) {
        const double u = cc * (dinv[i] * vv[i]);
        xout[i] = xin ? xin[i] + u : u;
        if (dout) dout[i] = u;
      }
    };
    auto step = [&](const double* xin, double* xout, double s1, double s2, const double* d_old, double* d_new) {
      ++n_step;
      const int j = n_step + (entry == ChebEntry::ITERATE ? 0 : 1);      // step of the recurrence
      if (entry != ChebEntry::ITERATE && !n_first) fail("a product step ahead of first()");
      if (xin == xout || !in_pair(xin) || !in_pair(xout)) fail("step(): passes ping-pong between x and tmp, out of place");
      if (j == 1) { if (s1 != 0.0 || s2 != c0 || d_old != nullptr || xin != src) fail("step 1 as a product step: (c1, c2) = (0, c0) on d_old = the iterate"); }
      else {
        if (s1 != c1[j] || s2 != c2[j]) fail("step(): coefficients");
        if (d_old != ((zero && j == 2) ? nullptr : d.data())) fail("step(): d_old is d, except after the first step from zero (the iterate itself)");
      }
      if (d_new != (j < k ? d.data() : nullptr)) fail("step(): d is stored exactly when another step follows");
      const Vec ax = matvec(xin);
      for (int i = 0; i < N; ++i) {
        const double dn = s1 * (d_old ? d_old[i] : xin[i]) + s2 * (dinv[i] * (b[i] - ax[i]));
        xout[i] = xin[i] + dn;
        if (d_new) d_new[i] = dn;
      }
    };
    const double* end = amgx::cheb_schedule(k, c0, c1, c2, entry, v, src, x.data(), tmp.data(), d.data(), first, step);
    if (n_first != (entry == ChebEntry::ITERATE ? 0 : 1)) fail("first() runs once, unless step 1 is a product step");
    if (n_step != amgx::cheb_passes(k, entry)) fail("product steps != cheb_passes");
    if (!in_pair(end)) fail("the result lies neither in x nor in tmp");
    const int passes = amgx::cheb_passes(k, entry);
    const bool placed = entry != ChebEntry::ITERATE || src == amgx::cheb_place(passes, x.data(), tmp.data());
    if ((end == x.data()) != placed) fail("a copy is needed exactly when the iterate was not placed by cheb_place");
    if (end != x.data()) x = tmp;                // the copy the caller makes
    for (int i = 0; i < N; ++i)
      if (!(std::fabs(x[i] - xr[i]) <= 1e-14 * std::fabs(xr[i]))) { fail("x differs from the literal recurrence"); break; }
  }
  // post_smooth's rule, as a number: t = x + P x_c goes to tmp for odd k, to x for even k
  double px, pt;
  for (int k = 1; k <= 8; ++k)
    if (amgx::cheb_place(amgx::cheb_passes(k, ChebEntry::ITERATE), &px, &pt) != ((k & 1) ? &pt : &px)) { std::printf("cheb_place, k=%d\n", k); ++bad; }
  if (amgx::cheb_passes(3, ChebEntry::ZERO) != 2 || amgx::cheb_passes(3, ChebEntry::RES_UPDATED) != 2 || amgx::cheb_passes(3, ChebEntry::ITERATE) != 3) {
    std::printf("cheb_passes\n");
    ++bad;
  }
  std::printf("cases=%d bad=%d\n", cases, bad);
  return bad ? 1 : 0;
}
"""


def test_cheb_schedule_host_program(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to compile cheb_schedule.hpp")
    src = tmp_path / "cheb_schedule_check.cpp"
    exe = tmp_path / "cheb_schedule_check"
    src.write_text(PROGRAM)
    inc = os.path.join(ROOT, "ngsamg_amd", "csrc", "device")
    cc = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", inc, "-o", str(exe), str(src)],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip().endswith("cases=30 bad=0"), run.stdout
