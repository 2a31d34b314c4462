"""down_nv_ok / down_nv_lds_bytes of ngsamg_amd/csrc/device/down_plan.hpp (which plans of the fused down launcher have a kernel on
2 or 4 interleaved vectors, AMGX_MULTI_FUSE_DOWN) compiled by a plain C++17 host compiler into a stand-alone program.

The program walks every (family, mode, workgroup size, lanes, EPT, width, on) of a grid that is wider than the value lists and
compares down_nv_ok with the rule written out independently here:
  * 512-lane workgroups only; widths 2 and 4 only; the plan is on;
  * sell family: one lane per row with EPT 4 or 6 in MODE 0 / 1 / 2; 2 / 4 / 8 lanes with EPT 4 in MODE 0 / 2 (MODE 1 has one lane);
  * windowed family: MODE 1, one lane, EPT 4 or 6;
  * local-window, diagonal and box-chunk images never.
For every admitted shape the LDS is 8 * (rows per chunk * width + EPT * 512) bytes, at most 40 KB and so below the 64 KB of a
workgroup."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include "down_plan.hpp"
#include <cstdio>

using namespace amgx;

int main() {
  int bad = 0;
  long cases = 0, admitted = 0;
  const int families[] = {DOWN_FAM_SELL, DOWN_FAM_WIN, DOWN_FAM_LW, DOWN_FAM_DIA, DOWN_FAM_DIA_BOX};
  const int sizes[] = {256, 512, 1024}, lanes_of[] = {1, 2, 3, 4, 8, 16}, epts[] = {2, 4, 5, 6, 8}, widths[] = {1, 2, 3, 4, 8};
  size_t lds_max = 0;
  for (int fam : families) for (int mode = 0; mode < 3; ++mode) for (int threads : sizes) for (int lanes : lanes_of) for (int ept : epts)
    for (int nv : widths) for (int on = 0; on < 2; ++on) {
      ++cases;
      DownPlan p;
      p.on = on != 0; p.family = fam; p.mode = mode; p.threads = threads; p.lanes = lanes; p.ept = ept;
      bool want = on && threads == 512 && (nv == 2 || nv == 4);
      if (fam == DOWN_FAM_SELL) {
        if (lanes == 1) want = want && (ept == 4 || ept == 6);
        else want = want && (lanes == 2 || lanes == 4 || lanes == 8) && ept == 4 && mode != 1;
      } else if (fam == DOWN_FAM_WIN) want = want && mode == 1 && lanes == 1 && (ept == 4 || ept == 6);
      else want = false;
      const bool got = down_nv_ok(p, nv);
      if (got != want) {
        std::printf("family=%d mode=%d threads=%d lanes=%d ept=%d nv=%d on=%d: down_nv_ok=%d, expected %d\n", fam, mode, threads, lanes, ept, nv, on, (int)got, (int)want);
        ++bad;
      }
      if (!got) continue;
      ++admitted;
      const size_t lds = down_nv_lds_bytes(p, nv), expect = 8u * ((size_t)(512 / lanes) * (size_t)nv + (size_t)ept * 512u);
      if (lds != expect || lds > 65536 || lds > 40960) {
        std::printf("family=%d mode=%d lanes=%d ept=%d nv=%d: lds=%zu, expected %zu (<= 40960)\n", fam, mode, lanes, ept, nv, lds, expect);
        ++bad;
      }
      if (lds > lds_max) lds_max = lds;
    }
  // the shapes the launcher names, one by one, and their closest neighbours
  constexpr auto plan = [](int fam, int mode, int threads, int lanes, int ept) {
    DownPlan p;
    p.on = true; p.family = fam; p.mode = mode; p.threads = threads; p.lanes = lanes; p.ept = ept;
    return p;
  };
  static_assert(down_nv_ok(plan(DOWN_FAM_SELL, 0, 512, 1, 6), 4) && down_nv_lds_bytes(plan(DOWN_FAM_SELL, 0, 512, 1, 6), 4) == 40960, "constexpr: usable where a kernel list is");
  for (int nv : {2, 4}) {
    for (int mode : {0, 1, 2}) for (int ept : {4, 6}) if (!down_nv_ok(plan(DOWN_FAM_SELL, mode, 512, 1, ept), nv)) { std::printf("sell one lane mode %d ept %d\n", mode, ept); ++bad; }
    for (int mode : {0, 2}) for (int lanes : {2, 4, 8}) {
      if (!down_nv_ok(plan(DOWN_FAM_SELL, mode, 512, lanes, 4), nv)) { std::printf("sell %d lanes mode %d\n", lanes, mode); ++bad; }
      if (down_nv_ok(plan(DOWN_FAM_SELL, mode, 512, lanes, 6), nv)) { std::printf("sell %d lanes with EPT 6\n", lanes); ++bad; }
    }
    for (int lanes : {2, 4, 8}) if (down_nv_ok(plan(DOWN_FAM_SELL, 1, 512, lanes, 4), nv)) { std::printf("MODE 1 with %d lanes\n", lanes); ++bad; }
    for (int ept : {4, 6}) {
      if (!down_nv_ok(plan(DOWN_FAM_WIN, 1, 512, 1, ept), nv)) { std::printf("win mode 1 ept %d\n", ept); ++bad; }
      if (down_nv_ok(plan(DOWN_FAM_WIN, 0, 512, 1, ept), nv) || down_nv_ok(plan(DOWN_FAM_WIN, 2, 512, 1, ept), nv)) { std::printf("win mode 0 / 2\n"); ++bad; }
      for (int threads : {256, 1024}) if (down_nv_ok(plan(DOWN_FAM_SELL, 0, threads, 1, ept), nv)) { std::printf("%d threads\n", threads); ++bad; }
      for (int fam : {DOWN_FAM_LW, DOWN_FAM_DIA, DOWN_FAM_DIA_BOX}) for (int lanes : {1, 2, 4})
        if (down_nv_ok(plan(fam, 0, 512, lanes, ept), nv) || down_nv_ok(plan(fam, 1, 512, lanes, ept), nv)) { std::printf("family %d\n", fam); ++bad; }
    }
  }
  if (lds_max != 40960) { std::printf("largest LDS %zu, expected 40960 (FB 512, EPT 6, NV 4)\n", lds_max); ++bad; }
  std::printf("cases=%ld admitted=%ld bad=%d\n", cases, admitted, bad);
  return bad ? 1 : 0;
}
"""


def build_and_run(tmp_path, flags=()):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to compile down_plan.hpp")
    src = tmp_path / "down_plan_nv_check.cpp"
    exe = tmp_path / "down_plan_nv_check"
    src.write_text(PROGRAM)
    inc = os.path.join(ROOT, "ngsamg_amd", "csrc", "device")
    cc = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *flags, "-I", inc, "-o", str(exe), str(src)],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    return subprocess.run([str(exe)], capture_output=True, text=True)


def test_down_nv_rule_host_program(tmp_path):
    run = build_and_run(tmp_path)
    assert run.returncode == 0, run.stdout + run.stderr
    last = run.stdout.strip().splitlines()[-1]
    fields = dict(f.split("=") for f in last.split())
    # 5 families x 3 modes x 3 sizes x 6 lane counts x 5 EPTs x 5 widths x on / off
    assert int(fields["cases"]) == 5 * 3 * 3 * 6 * 5 * 5 * 2 and int(fields["bad"]) == 0, run.stdout
    # sell: 3 modes x 2 EPTs (one lane) + 2 modes x 3 lane counts; win: 2 EPTs; each at two widths
    assert int(fields["admitted"]) == 2 * (3 * 2 + 2 * 3 + 2), run.stdout
