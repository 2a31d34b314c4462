"""AMGX_MULTI_FUSE_F32: the fusion rule with the fact MultiLevelFacts::f32_ok, the Python words and the C value.

multi_rule.hpp is compiled by a plain C++17 host compiler, as tests/test_multi_rule_cpu.py does.  The program below carries a copy
of multi_level_reason as it was before the fact existed (with sgs_f32) and checks
  * fact false: every combination of the facts the rule reads, rules 0-3, gives the copy's answer;
  * fact true: a decision differs from the copy's only where the copy answered "single-precision Gauss-Seidel images" -- scalar levels
    under rules 2 and 3, block levels under rule 3 -- and the new answer is what the copy gives with the two image facts cleared (the
    next question in line); every one of these classes occurs;
  * jacobi_f32 refuses under every rule whatever the new fact says."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include "multi_rule.hpp"
#include <cstdio>
#include <cstring>
using namespace amgx;
using F = MultiLevelFacts;

// multi_level_reason as it was before the fact f32_ok existed
static const char* parent_reason(int rule, const F& f) {
  const bool base = rule == 0;
  const bool jacobi = f.sm_type == AMGX_SM_JACOBI, cheby = f.sm_type == AMGX_SM_CHEBY;
  const bool gs = f.smoothed && rule >= 2 && f.sm_type == AMGX_SM_GS;
  auto smoother = [&]() -> const char* {
    if (!f.smoothed) return nullptr;
    if (rule >= 2 && f.sm_type == AMGX_SM_BGS) return "block Gauss-Seidel (bgs) smoother";
    if (rule == 2 && gs && f.bs != 1) return "Gauss-Seidel on a block level";
    if (!(jacobi || (cheby && !base) || gs))
      return base ? "smoother is not Jacobi" : rule == 1 ? "smoother is not Jacobi or Chebyshev" : "smoother is not Jacobi, Chebyshev or Gauss-Seidel";
    if (!f.plain) return "sm_steps > 1 or sm_symm";
    if (cheby && (f.cheb_degree < 1 || f.cheb_degree > 8)) return "Chebyshev level without coefficients";
    return nullptr;
  };
  auto level = [&]() -> const char* {
    if (base && f.bs != 1) return "block level";
    if (f.bs != 1 && f.bs != 2 && f.bs != 3 && f.bs != 6) return "block size is not 1, 2, 3 or 6";
    if (!f.square) return "ghost columns";
    if (f.permuted) return "renumbered level";
    if (f.jacobi_f32) return "single-precision Jacobi images";
    if (gs && !f.empty) {
      if (rule >= 3 && f.gs_f32) return "single-precision Gauss-Seidel images";
      if (f.sgs_f32) return "single-precision Gauss-Seidel images";
      if (!(f.bs == 1 ? f.sweep_ok : f.block_sweep_ok)) return "Gauss-Seidel sweep form without a multi-vector kernel";
      if (f.bs != 1 && !f.block_sweep_fits) return "sweep block too large for the multi-vector sweep";
    }
    if (!f.empty && !(base ? f.a_scalar : f.a_level)) return "level matrix format";
    return nullptr;
  };
  const char* why = base ? level() : smoother();
  if (!why) why = base ? smoother() : level();
  if (!why && f.smoothed && !f.empty && !(base ? f.t_scalar : f.t_transfer)) why = "transfer format";
  return why;
}
static bool same(const char* a, const char* b) { return (!a && !b) || (a && b && !std::strcmp(a, b)); }
static const char* show(const char* a) { return a ? a : "(admitted)"; }
static const char* const GS32 = "single-precision Gauss-Seidel images";

int main() {
  if (F().f32_ok) { std::printf("the fact does not default to false\n"); return 1; }
  long n = 0, changed[4][2] = {{0, 0}, {0, 0}, {0, 0}, {0, 0}}, admitted_new = 0, jac = 0;       // changed[rule][block level]
  for (int bs : {1, 2, 3, 4, 6}) for (int sm = 0; sm < 4; ++sm) for (int deg : {0, 2, 9}) for (int bits = 0; bits < (1 << 15); ++bits) {
    F f;
    f.bs = bs; f.sm_type = sm; f.cheb_degree = deg;
    f.smoothed = bits & 1; f.plain = bits & 2; f.empty = bits & 4; f.square = bits & 8; f.permuted = bits & 16; f.jacobi_f32 = bits & 32; f.gs_f32 = bits & 64;
    f.a_scalar = bits & 128; f.a_level = bits & 256; f.t_scalar = bits & 512; f.t_transfer = bits & 1024;
    f.sweep_ok = bits & 2048; f.block_sweep_ok = bits & 4096; f.block_sweep_fits = bits & 8192; f.sgs_f32 = bits & 16384;
    for (int rule = 0; rule < 4; ++rule, ++n) {
      const char* old = parent_reason(rule, f);
      f.f32_ok = false;
      if (!same(multi_level_reason(rule, f), old)) {
        std::printf("fact false, rule %d bs %d sm %d deg %d bits %#x: \"%s\", the parent says \"%s\"\n", rule, bs, sm, deg, bits, show(multi_level_reason(rule, f)), show(old));
        return 1;
      }
      f.f32_ok = true;
      const char* now = multi_level_reason(rule, f);
      f.f32_ok = false;
      if (f.jacobi_f32 && !now) { std::printf("jacobi_f32 admitted under rule %d\n", rule); return 1; }
      if (f.jacobi_f32 && now && !std::strcmp(now, "single-precision Jacobi images")) ++jac;
      if (same(now, old)) continue;
      // only a refusal for Gauss-Seidel images may change, and only to the answer of the questions behind it
      if (!old || std::strcmp(old, GS32)) { std::printf("fact true changes \"%s\" to \"%s\" (rule %d bs %d sm %d bits %#x)\n", show(old), show(now), rule, bs, sm, bits); return 1; }
      F g = f;
      g.gs_f32 = g.sgs_f32 = false;
      if (!same(now, parent_reason(rule, g))) { std::printf("fact true: \"%s\", expected \"%s\" (rule %d bs %d sm %d bits %#x)\n", show(now), show(parent_reason(rule, g)), rule, bs, sm, bits); return 1; }
      if (now && !std::strcmp(now, GS32)) { std::printf("the refusal stays a change?\n"); return 1; }
      ++changed[rule][bs != 1];
      admitted_new += !now;
    }
  }
  // where decisions change: scalar levels under rules 2 and 3, block levels under rule 3, nothing else
  if (changed[0][0] || changed[0][1] || changed[1][0] || changed[1][1] || changed[2][1]) { std::printf("a decision changed under rule 0 / 1 or on a block level under rule 2\n"); return 1; }
  if (!changed[2][0] || !changed[3][0] || !changed[3][1] || !admitted_new || !jac) { std::printf("a class of changes is empty: %ld %ld %ld %ld %ld\n", changed[2][0], changed[3][0], changed[3][1], admitted_new, jac); return 1; }
  // a handle: a scalar Gauss-Seidel level with float images above a coarsest level
  F lev[2];
  for (F& f : lev) { f.a_scalar = f.a_level = f.t_scalar = f.t_transfer = true; f.sm_type = AMGX_SM_GS; f.sweep_ok = true; }
  lev[0].smoothed = true; lev[0].sgs_f32 = true;
  for (int rule = 2; rule < 4; ++rule) {
    MultiDecision d = multi_handle_rule(rule, true, lev, 2);
    if (d.fused != 0 || d.why != "single-precision Gauss-Seidel images (level 0)") { std::printf("rule %d without the fact: '%s'\n", rule, d.why.c_str()); return 1; }
    lev[0].f32_ok = true;
    d = multi_handle_rule(rule, true, lev, 2);
    if (d.fused != 1 || !d.why.empty()) { std::printf("rule %d with the fact: '%s'\n", rule, d.why.c_str()); return 1; }
    lev[0].jacobi_f32 = true;
    d = multi_handle_rule(rule, true, lev, 2);
    if (d.fused != 0 || d.why != "single-precision Jacobi images (level 0)") { std::printf("rule %d with jacobi_f32: '%s'\n", rule, d.why.c_str()); return 1; }
    lev[0].jacobi_f32 = false; lev[0].f32_ok = false;
  }
  // the flag is none of the rule flags: it picks no rule
  int fused[4] = {0, 0, 1, 1};
  if (multi_asked_rule(AMGX_MULTI_FUSE_F32) != 0 || multi_runs_fused(AMGX_MULTI_FUSE_F32, fused) || (MULTI_RULE_FLAGS & AMGX_MULTI_FUSE_F32)) { std::printf("the flag widens the rule\n"); return 1; }
  if (!multi_runs_fused(AMGX_MULTI_FUSE_F32 | AMGX_MULTI_FUSE_GS, fused) || multi_rule_in_force(AMGX_MULTI_FUSE_F32 | AMGX_MULTI_FUSE_GS, fused) != 2) { std::printf("the flag disturbs the rule in force\n"); return 1; }
  std::printf("ok %ld scalar2=%ld scalar3=%ld block3=%ld admitted=%ld value=%d\n", n, changed[2][0], changed[3][0], changed[3][1], admitted_new, (int)AMGX_MULTI_FUSE_F32);
  return 0;
}
"""


def test_rule_with_and_without_the_fact(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to compile multi_rule.hpp")
    src, exe = tmp_path / "rule_f32.cpp", tmp_path / "rule_f32"
    src.write_text(PROGRAM)
    cc = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "ngsamg_amd", "csrc", "device"),
                         "-o", str(exe), str(src)], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout + out.stderr
    fields = dict(f.split("=") for f in out.stdout.split()[2:])
    assert int(out.stdout.split()[1]) == 5 * 4 * 3 * 2 ** 15 * 4, out.stdout
    assert int(fields["value"]) == 2048 and all(int(fields[k]) > 0 for k in ("scalar2", "scalar3", "block3", "admitted")), out.stdout


def test_python_words_and_values():
    from ngsamg_amd import _lib
    from ngsamg_amd._lib import NgsAMGError
    from ngsamg_amd.device import check_fuse
    assert _lib.AMGX_MULTI_FUSE_F32 == 2048
    for word in ("gs", "gs_block", "gs+down", "gs_block+down"):
        assert check_fuse(word + "+f32") == check_fuse(word) | _lib.AMGX_MULTI_FUSE_F32, word
        assert check_fuse(word) & _lib.AMGX_MULTI_FUSE_F32 == 0, word
    assert check_fuse("gs+f32") == 64 | 128 | 2048 and check_fuse("gs_block+f32") == 64 | 128 | 256 | 2048
    assert check_fuse("gs+down+f32") == 64 | 128 | 512 | 2048 and check_fuse("gs_block+down+f32") == 64 | 128 | 256 | 512 | 2048
    # every other word and value is what it was
    assert [check_fuse(w) for w in (False, True, "gs", "gs_block", "down", "gs+down", "gs_block+down", "down_dia", "gs+down_dia", "gs_block+down_dia")] == \
        [0, 64, 192, 448, 576, 704, 960, 1600, 1728, 1984]
    for bad in ("f32", "+f32", "down+f32", "gs+f32+down", "gs+down_dia+f32", "GS+F32", "gs +f32", 2048, None, 1):
        with pytest.raises(NgsAMGError, match="fuse: need True, False") as ei:
            check_fuse(bad)
        assert '"gs+f32"' in str(ei.value) and repr(bad) in str(ei.value), str(ei.value)


def test_header_declares_the_value():
    text = open(os.path.join(ROOT, "include", "amgx.h")).read()
    m = re.search(r"\bAMGX_MULTI_FUSE_F32\s*=\s*(\d+)", text)
    assert m and int(m.group(1)) == 2048, m
    src = ('#include "amgx.h"\n_Static_assert(AMGX_MULTI_FUSE_F32 == 2048, "value");\n'
           '_Static_assert((AMGX_MULTI_FUSE_F32 & (AMGX_MULTI_FUSE | AMGX_MULTI_FUSE_GS | AMGX_MULTI_FUSE_GS_BLOCK | AMGX_MULTI_FUSE_DOWN | '
           'AMGX_MULTI_FUSE_DOWN_DIA | AMGX_MULTI_INTERLEAVED | AMGX_DEVICE_PTR | AMGX_NO_GRAPH)) == 0, "a bit of its own");\nint main(void){return 0;}\n')
    cc = subprocess.run(["gcc", "-std=c11", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c", "-"], input=src,
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
