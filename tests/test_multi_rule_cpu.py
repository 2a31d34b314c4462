"""The fusion rule of the multi-vector calls (ngsamg_amd/csrc/device/multi_rule.hpp) compiled by
a plain C++17 host compiler into a stand-alone program.

multi_level_reason states every check once and reads the four rules (no flag, AMGX_MULTI_FUSE, ..._GS, ..._GS_BLOCK) as differences.
The program below states them the other way: each rule as its own straight-line function on the facts, in the order in which
amgx_multi_note has always answered.  The four copies are deliberate: they are the independent statement of the contract.
  * level rule: every MultiLevelFacts over bs in {1, 2, 3, 4, 6}, every AMGX_SM_* value, cheb_degree in {0, 2, 8, 9} and both values
    of the fourteen yes / no facts -- the same string (or both none) under each rule;
  * inclusion: on the facts a handle can produce, a level admitted under rule r is admitted under rule r + 1;
  * handle rule: first failing level named, suffix " (level l)", "cycle is not V" first and without a level, the coarsest level not
    asked about smoother or transfers, "" and fused = 1 where every level passes;
  * flags: every subset of the five flag bits on every monotone fused[4] against the two chains of conditions written out here;
  * multi_groups: k ones unfused; fused the greedy cut into 4, 2, 1."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include "multi_rule.hpp"
#include <cstdio>
#include <cstring>
#include <vector>

using namespace amgx;
using F = MultiLevelFacts;

static bool size_ok(int bs) { return bs == 1 || bs == 2 || bs == 3 || bs == 6; }
static bool cheb_bad(const F& f) { return f.sm_type == AMGX_SM_CHEBY && (f.cheb_degree < 1 || f.cheb_degree > 8); }

// ---- the four rules, each on its own
static const char* rule0(const F& f) {
  if (f.bs != 1) return "block level";
  if (!f.square) return "ghost columns";
  if (f.permuted) return "renumbered level";
  if (f.jacobi_f32) return "single-precision Jacobi images";
  if (!f.empty && !f.a_scalar) return "level matrix format";
  if (!f.smoothed) return nullptr;
  if (f.sm_type != AMGX_SM_JACOBI) return "smoother is not Jacobi";
  if (!f.plain) return "sm_steps > 1 or sm_symm";
  if (!f.empty && !f.t_scalar) return "transfer format";
  return nullptr;
}
static const char* rule1(const F& f) {
  if (f.smoothed) {
    if (f.sm_type != AMGX_SM_JACOBI && f.sm_type != AMGX_SM_CHEBY) return "smoother is not Jacobi or Chebyshev";
    if (!f.plain) return "sm_steps > 1 or sm_symm";
    if (cheb_bad(f)) return "Chebyshev level without coefficients";
  }
  if (!size_ok(f.bs)) return "block size is not 1, 2, 3 or 6";
  if (!f.square) return "ghost columns";
  if (f.permuted) return "renumbered level";
  if (f.jacobi_f32) return "single-precision Jacobi images";
  if (!f.empty && !f.a_level) return "level matrix format";
  if (f.smoothed && !f.empty && !f.t_transfer) return "transfer format";
  return nullptr;
}
static const char* rule2(const F& f) {
  const bool gs = f.smoothed && f.sm_type == AMGX_SM_GS;
  if (f.smoothed) {
    if (f.sm_type == AMGX_SM_BGS) return "block Gauss-Seidel (bgs) smoother";
    if (gs && f.bs != 1) return "Gauss-Seidel on a block level";
    if (!gs && f.sm_type != AMGX_SM_JACOBI && f.sm_type != AMGX_SM_CHEBY) return "smoother is not Jacobi, Chebyshev or Gauss-Seidel";
    if (!f.plain) return "sm_steps > 1 or sm_symm";
    if (cheb_bad(f)) return "Chebyshev level without coefficients";
  }
  if (!size_ok(f.bs)) return "block size is not 1, 2, 3 or 6";
  if (!f.square) return "ghost columns";
  if (f.permuted) return "renumbered level";
  if (f.jacobi_f32) return "single-precision Jacobi images";
  if (gs && !f.empty && !f.sweep_ok) return "Gauss-Seidel sweep form without a multi-vector kernel";
  if (!f.empty && !f.a_level) return "level matrix format";
  if (f.smoothed && !f.empty && !f.t_transfer) return "transfer format";
  return nullptr;
}
static const char* rule3(const F& f) {
  const bool gs = f.smoothed && f.sm_type == AMGX_SM_GS;
  if (f.smoothed) {
    if (f.sm_type == AMGX_SM_BGS) return "block Gauss-Seidel (bgs) smoother";
    if (!gs && f.sm_type != AMGX_SM_JACOBI && f.sm_type != AMGX_SM_CHEBY) return "smoother is not Jacobi, Chebyshev or Gauss-Seidel";
    if (!f.plain) return "sm_steps > 1 or sm_symm";
    if (cheb_bad(f)) return "Chebyshev level without coefficients";
  }
  if (!size_ok(f.bs)) return "block size is not 1, 2, 3 or 6";
  if (!f.square) return "ghost columns";
  if (f.permuted) return "renumbered level";
  if (f.jacobi_f32) return "single-precision Jacobi images";
  if (gs && !f.empty) {
    if (f.gs_f32) return "single-precision Gauss-Seidel images";
    if (!(f.bs == 1 ? f.sweep_ok : f.block_sweep_ok)) return "Gauss-Seidel sweep form without a multi-vector kernel";
    if (f.bs != 1 && !f.block_sweep_fits) return "sweep block too large for the multi-vector sweep";
  }
  if (!f.empty && !f.a_level) return "level matrix format";
  if (f.smoothed && !f.empty && !f.t_transfer) return "transfer format";
  return nullptr;
}
static const char* (*const RULES[4])(const F&) = {rule0, rule1, rule2, rule3};

static bool same(const char* a, const char* b) { return (!a && !b) || (a && b && std::strcmp(a, b) == 0); }
static const char* show(const char* a) { return a ? a : "(admitted)"; }

// the facts amgx_create can produce: a scalar format is a level format and a transfer format; the sweep answers imply what
// Handle::multi_sweep_ok / multi_block_sweep_ok ask first; single-precision Gauss-Seidel images exist on block levels only
static bool producible(const F& f) {
  if (f.a_scalar && !f.a_level) return false;
  if (f.t_scalar && !f.t_transfer) return false;
  const bool sweepable = f.sm_type == AMGX_SM_GS && f.square && f.plain;
  if (f.sweep_ok && !(f.bs == 1 && sweepable)) return false;
  if (f.block_sweep_ok && !((f.bs == 2 || f.bs == 3 || f.bs == 6) && sweepable && !f.gs_f32)) return false;
  if (f.gs_f32 && f.bs == 1) return false;
  return true;
}

static F good(int sm_type, bool smoothed) {       // a scalar level every rule admits with a Jacobi smoother
  F f;
  f.smoothed = smoothed; f.sm_type = sm_type; f.cheb_degree = 3;
  f.a_scalar = f.a_level = f.t_scalar = f.t_transfer = true;
  return f;
}

int main() {
  long bad = 0, cases = 0, admitted[4] = {0, 0, 0, 0}, producible_cases = 0;
  auto fail = [&](const char* what) { if (++bad <= 20) std::printf("%s\n", what); };
  char msg[512];

  // ---- the level rule, exhaustively
  const int sizes[] = {1, 2, 3, 4, 6}, smoothers[] = {AMGX_SM_JACOBI, AMGX_SM_GS, AMGX_SM_BGS, AMGX_SM_CHEBY}, degrees[] = {0, 2, 8, 9};
  for (int bs : sizes) for (int sm : smoothers) for (int deg : degrees) for (unsigned bits = 0; bits < (1u << 14); ++bits) {
    F f;
    f.bs = bs; f.sm_type = sm; f.cheb_degree = deg;
    f.smoothed = bits & 1; f.plain = bits & 2; f.empty = bits & 4; f.square = bits & 8; f.permuted = bits & 16; f.jacobi_f32 = bits & 32; f.gs_f32 = bits & 64;
    f.a_scalar = bits & 128; f.a_level = bits & 256; f.t_scalar = bits & 512; f.t_transfer = bits & 1024;
    f.sweep_ok = bits & 2048; f.block_sweep_ok = bits & 4096; f.block_sweep_fits = bits & 8192;
    ++cases;
    const char* got[4];
    for (int r = 0; r < 4; ++r) {
      got[r] = multi_level_reason(r, f);
      const char* want = RULES[r](f);
      admitted[r] += !got[r];
      if (!same(got[r], want)) {
        std::snprintf(msg, sizeof msg, "rule %d bs=%d sm=%d deg=%d bits=%#x: \"%s\", expected \"%s\"", r, bs, sm, deg, bits, show(got[r]), show(want));
        fail(msg);
      }
    }
    if (!producible(f)) continue;
    ++producible_cases;
    for (int r = 0; r < 3; ++r)
      if (!got[r] && got[r + 1]) {
        std::snprintf(msg, sizeof msg, "inclusion: bs=%d sm=%d deg=%d bits=%#x admitted under rule %d, \"%s\" under rule %d", bs, sm, deg, bits, r, got[r + 1], r + 1);
        fail(msg);
      }
  }

  // ---- the handle rule
  auto expect = [&](const char* what, const MultiDecision& d, int fused, const std::string& why) {
    if (d.fused != fused || d.why != why) {
      std::snprintf(msg, sizeof msg, "%s: fused=%d \"%s\", expected %d \"%s\"", what, d.fused, d.why.c_str(), fused, why.c_str());
      fail(msg);
    }
  };
  for (int r = 0; r < 4; ++r) for (int L : {2, 3}) {
    std::vector<F> lev(L, good(AMGX_SM_JACOBI, true));
    // the coarsest level is asked neither about its smoother nor about its transfers
    F& last = lev[L - 1];
    last.smoothed = false; last.sm_type = AMGX_SM_BGS; last.plain = false; last.cheb_degree = 0; last.t_scalar = last.t_transfer = false;
    last.sweep_ok = last.block_sweep_ok = last.block_sweep_fits = false;
    expect("all admitted", multi_handle_rule(r, true, lev.data(), L), 1, "");
    expect("not V", multi_handle_rule(r, false, lev.data(), L), 0, "cycle is not V");
    for (int l = 0; l < L; ++l) {                  // one failing level; then a second one behind it, which must not be named
      std::vector<F> one = lev;
      one[l].permuted = true;
      expect("one renumbered level", multi_handle_rule(r, true, one.data(), L), 0, "renumbered level (level " + std::to_string(l) + ")");
      expect("not V wins", multi_handle_rule(r, false, one.data(), L), 0, "cycle is not V");
      for (int m = l + 1; m < L; ++m) {
        std::vector<F> two = one;
        two[m].square = false;
        expect("first of two", multi_handle_rule(r, true, two.data(), L), 0, "renumbered level (level " + std::to_string(l) + ")");
      }
      if (l + 1 < L) {                             // a smoothed level is asked: each rule in its own words
        std::vector<F> sm = lev;
        sm[l].sm_type = AMGX_SM_BGS;
        expect("bgs level", multi_handle_rule(r, true, sm.data(), L), 0, std::string(RULES[r](sm[l])) + " (level " + std::to_string(l) + ")");
        sm[l] = lev[l];
        sm[l].t_scalar = sm[l].t_transfer = false;
        expect("transfer", multi_handle_rule(r, true, sm.data(), L), 0, "transfer format (level " + std::to_string(l) + ")");
      }
    }
  }
  expect("no level", multi_handle_rule(0, true, nullptr, 0), 1, "");

  // ---- the flags: every subset of the five bits on every monotone fused[4]
  const int bit[5] = {AMGX_MULTI_FUSE, AMGX_MULTI_FUSE_GS, AMGX_MULTI_FUSE_GS_BLOCK, AMGX_MULTI_FUSE_DOWN, AMGX_MULTI_FUSE_DOWN_DIA};
  long flag_cases = 0;
  for (int first = 0; first <= 4; ++first) for (int sub = 0; sub < 32; ++sub) {      // fused[r] = r >= first
    int fused[4], flags = AMGX_MULTI_INTERLEAVED;                                     // (a bit that is none of the five)
    for (int r = 0; r < 4; ++r) fused[r] = r >= first;
    for (int i = 0; i < 5; ++i) if (sub >> i & 1) flags |= bit[i];
    const bool block_flag = flags & AMGX_MULTI_FUSE_GS_BLOCK, gs_flag = flags & (AMGX_MULTI_FUSE_GS | AMGX_MULTI_FUSE_GS_BLOCK);
    const bool fuse_flag = flags & (AMGX_MULTI_FUSE | AMGX_MULTI_FUSE_GS | AMGX_MULTI_FUSE_GS_BLOCK);
    const bool fz = fused[0] == 1 || (fuse_flag && fused[1] == 1) || (gs_flag && fused[2] == 1) || (block_flag && fused[3] == 1);
    int rule;
    if (fused[0] == 1 || !fuse_flag) rule = 0;
    else if (block_flag && fused[2] != 1 && fused[1] != 1) rule = 3;
    else rule = gs_flag && fused[1] != 1 ? 2 : 1;
    ++flag_cases;
    if (multi_rule_in_force(flags, fused) != rule || multi_runs_fused(flags, fused) != fz) {
      std::snprintf(msg, sizeof msg, "flags %#x first fused rule %d: rule %d fused %d, expected %d %d", flags, first, multi_rule_in_force(flags, fused),
                    (int)multi_runs_fused(flags, fused), rule, (int)fz);
      fail(msg);
    }
  }

  // ---- multi_groups
  for (int k = 1; k <= AMGX_MULTI_MAX; ++k) {
    int32_t w[AMGX_MULTI_MAX];
    int n = multi_groups(k, false, w);
    bool ok = n == k;
    for (int g = 0; g < n && ok; ++g) ok = w[g] == 1;
    if (!ok) { std::snprintf(msg, sizeof msg, "multi_groups(%d, unfused)", k); fail(msg); }
    n = multi_groups(k, true, w);
    int sum = 0, singles = 0, left = k;
    ok = true;
    for (int g = 0; g < n; ++g) {
      const int greedy = left >= 4 ? 4 : left >= 2 ? 2 : 1;
      ok = ok && w[g] == greedy;
      sum += w[g]; singles += w[g] == 1; left -= w[g];
    }
    if (!ok || sum != k || singles > 1) { std::snprintf(msg, sizeof msg, "multi_groups(%d, fused)", k); fail(msg); }
  }

  std::printf("cases=%ld producible=%ld admitted0=%ld admitted1=%ld admitted2=%ld admitted3=%ld flag_cases=%ld bad=%ld\n", cases, producible_cases,
              admitted[0], admitted[1], admitted[2], admitted[3], flag_cases, bad);
  return bad ? 1 : 0;
}
"""


def build_and_run(tmp_path, flags=()):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to compile multi_rule.hpp")
    src = tmp_path / "multi_rule_check.cpp"
    exe = tmp_path / "multi_rule_check"
    src.write_text(PROGRAM)
    inc = os.path.join(ROOT, "ngsamg_amd", "csrc", "device")
    cc = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *flags, "-I", inc, "-o", str(exe), str(src)],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    return subprocess.run([str(exe)], capture_output=True, text=True)


def test_multi_rule_host_program(tmp_path):
    run = build_and_run(tmp_path)
    assert run.returncode == 0, run.stdout + run.stderr
    last = run.stdout.strip().splitlines()[-1]
    fields = dict(f.split("=") for f in last.split())
    # 5 block sizes x 4 smoothers x 4 degrees x 2^14 yes / no facts; 5 monotone fused[4] x 2^5 flag subsets
    assert int(fields["cases"]) == 5 * 4 * 4 * 2 ** 14 and int(fields["flag_cases"]) == 5 * 32 and int(fields["bad"]) == 0, run.stdout
    # the grid is not degenerate: every rule admits some levels and refuses others, and the inclusion check had facts to look at
    assert all(0 < int(fields[f"admitted{r}"]) < int(fields["cases"]) for r in range(4)), run.stdout
    assert int(fields["producible"]) > 0, run.stdout


def test_multi_rule_header_is_host_only():
    text = open(os.path.join(ROOT, "ngsamg_amd", "csrc", "device", "multi_rule.hpp")).read()
    includes = [line.split()[1] for line in text.splitlines() if line.startswith("#include")]
    assert includes == ["<cstdint>", "<string>", '"../../../include/amgx.h"'], includes
