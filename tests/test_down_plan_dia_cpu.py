"""down_nv_dia_ok / down_nv_dia_lds_bytes of ngsamg_amd/csrc/device/down_plan.hpp (which diagonal-image plans of the fused down
launcher have a kernel on 2 or 4 interleaved vectors, AMGX_MULTI_FUSE_DOWN_DIA) compiled by a plain C++17 host compiler
into a stand-alone program.

The program walks every (family, mode, workgroup size, lanes, EPT, diagonals, box rows, entries, width, on) of a grid that is wider
than the value lists and compares down_nv_dia_ok with the rule written out independently here:
  * the plan is on, widths 2 and 4 only, MODE 0 only, 512-lane workgroups, one lane per row;
  * 512-row chunks: 1 .. 8 upper diagonals, EPT 4 or 6; LDS 8 * (512 * width + EPT * 512) bytes, at most 40 KB;
  * box chunks: 2 .. 7 upper diagonals; LDS 8 * (box rows * width + max(box rows * width, entries)) bytes, at most 160 KB;
  * every other family never;
and down_nv_ok keeps refusing both diagonal families whatever the rest of the plan says."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include "down_plan.hpp"
#include <cstdio>

using namespace amgx;

static size_t lds_expected(int fam, int ept, long box_rows, long entries, int nv) {
  if (fam == DOWN_FAM_DIA) return 8u * (512u * (size_t)nv + (size_t)ept * 512u);
  const size_t xs = (size_t)box_rows * (size_t)nv, e = (size_t)entries;
  return 8u * (xs + (xs > e ? xs : e));
}

int main() {
  int bad = 0;
  long cases = 0, admitted = 0, admitted_dia = 0, admitted_box = 0;
  const int families[] = {DOWN_FAM_SELL, DOWN_FAM_WIN, DOWN_FAM_LW, DOWN_FAM_DIA, DOWN_FAM_DIA_BOX};
  const int sizes[] = {256, 512, 1024}, lanes_of[] = {1, 2, 4}, epts[] = {2, 4, 5, 6, 8}, diags_of[] = {0, 1, 2, 3, 5, 7, 8, 9}, widths[] = {1, 2, 3, 4, 8};
  // (box rows, entries of the fullest box): cfg 2, the fullest box a level can have, a thin box, and two that no workgroup can hold
  const long boxes[][2] = {{1720, 6650}, {2048, 8192}, {48, 100}, {328, 1640}, {2048, 20000}, {6000, 100}};
  size_t dia_max = 0, box_max = 0;
  for (int fam : families) for (int mode = 0; mode < 3; ++mode) for (int threads : sizes) for (int lanes : lanes_of) for (int ept : epts)
    for (int diags : diags_of) for (const auto& bx : boxes) for (int nv : widths) for (int on = 0; on < 2; ++on) {
      ++cases;
      DownPlan p;
      p.on = on != 0; p.family = fam; p.mode = mode; p.threads = threads; p.lanes = lanes; p.ept = ept; p.diags = diags;
      p.box_rows = bx[0]; p.max_entries = bx[1];
      bool want = on && (nv == 2 || nv == 4) && mode == 0 && threads == 512 && lanes == 1;
      if (fam == DOWN_FAM_DIA) want = want && diags >= 1 && diags <= 8 && (ept == 4 || ept == 6);
      else if (fam == DOWN_FAM_DIA_BOX) want = want && diags >= 2 && diags <= 7;
      else want = false;
      if (want) want = lds_expected(fam, ept, bx[0], bx[1], nv) <= 163840;
      const bool got = down_nv_dia_ok(p, nv);
      if (got != want) {
        std::printf("family=%d mode=%d threads=%d lanes=%d ept=%d diags=%d box=%ld/%ld nv=%d on=%d: down_nv_dia_ok=%d, expected %d\n", fam, mode, threads, lanes, ept,
                    diags, bx[0], bx[1], nv, on, (int)got, (int)want);
        ++bad;
      }
      // the rule of AMGX_MULTI_FUSE_DOWN alone keeps refusing both families
      if ((fam == DOWN_FAM_DIA || fam == DOWN_FAM_DIA_BOX) && down_nv_ok(p, nv)) { std::printf("down_nv_ok admits family %d\n", fam); ++bad; }
      if (!got) continue;
      ++admitted;
      const size_t lds = down_nv_dia_lds_bytes(p, nv), expect = lds_expected(fam, ept, bx[0], bx[1], nv);
      if (lds != expect || lds > 163840) { std::printf("family=%d ept=%d box=%ld/%ld nv=%d: lds=%zu, expected %zu\n", fam, ept, bx[0], bx[1], nv, lds, expect); ++bad; }
      if (fam == DOWN_FAM_DIA) { ++admitted_dia; if (lds > 40960) { std::printf("row chunks: lds=%zu > 40960\n", lds); ++bad; } if (lds > dia_max) dia_max = lds; }
      else { ++admitted_box; if (lds > box_max) box_max = lds; }
    }
  constexpr auto dia = [](int diags, int ept) {
    DownPlan p;
    p.on = true; p.family = DOWN_FAM_DIA; p.mode = 0; p.threads = 512; p.lanes = 1; p.ept = ept; p.diags = diags;
    return p;
  };
  constexpr auto box = [](int diags, long rows, long entries) {
    DownPlan p;
    p.on = true; p.family = DOWN_FAM_DIA_BOX; p.mode = 0; p.threads = 512; p.lanes = 1; p.ept = 4; p.diags = diags; p.box_rows = rows; p.max_entries = entries;
    return p;
  };
  static_assert(down_nv_dia_ok(dia(7, 6), 4) && down_nv_dia_lds_bytes(dia(7, 6), 4) == 40960, "constexpr: usable where a kernel list is");
  static_assert(DOWN_NV_DIA_LDS_MAX == 163840, "160 KiB");
  // level 0 of cfg 2: 1720-row boxes with about 6650 entries
  if (down_nv_dia_lds_bytes(box(7, 1720, 6650), 2) != 80720) { std::printf("cfg 2 box at NV 2: %zu\n", down_nv_dia_lds_bytes(box(7, 1720, 6650), 2)); ++bad; }
  if (down_nv_dia_lds_bytes(box(7, 1720, 6650), 4) != 110080) { std::printf("cfg 2 box at NV 4: %zu\n", down_nv_dia_lds_bytes(box(7, 1720, 6650), 4)); ++bad; }
  // the fullest box a level can have: 2048 rows, entries up to the 10240 - 2048 doubles the single-vector kernel leaves them
  for (int nv : {2, 4}) {
    const size_t worst = down_nv_dia_lds_bytes(box(7, 2048, 10240 - 2048), nv);
    if (worst >= 163840 || !down_nv_dia_ok(box(7, 2048, 10240 - 2048), nv)) { std::printf("2048-row box at NV %d: %zu\n", nv, worst); ++bad; }
  }
  // every box the single-vector kernel takes (rows <= 2048, entries <= 10240 - rows) passes the bound: a guard, not a filter
  for (long rows = 48; rows <= 2048; rows += 8)
    if (!down_nv_dia_ok(box(3, rows, 10240 - rows), 4) || !down_nv_dia_ok(box(3, rows, 10240 - rows), 2)) { std::printf("box of %ld rows refused\n", rows); ++bad; }
  // the bound itself
  if (down_nv_dia_ok(box(7, 2048, 20000), 2) || down_nv_dia_ok(box(7, 6000, 100), 4)) { std::printf("a box beyond 160 KiB is admitted\n"); ++bad; }
  if (!down_nv_dia_ok(box(7, 5120, 100), 2) || down_nv_dia_ok(box(7, 5121, 100), 2)) { std::printf("the bound is not 163840\n"); ++bad; }
  // neighbours of the lists
  for (int nv : {2, 4}) {
    if (down_nv_dia_ok(dia(0, 4), nv) || down_nv_dia_ok(dia(9, 4), nv) || down_nv_dia_ok(dia(3, 5), nv) || down_nv_dia_ok(dia(3, 8), nv)) { std::printf("row chunks: list neighbours\n"); ++bad; }
    if (down_nv_dia_ok(box(1, 328, 1640), nv) || down_nv_dia_ok(box(8, 328, 1640), nv)) { std::printf("box chunks: list neighbours\n"); ++bad; }
    for (int k = 1; k <= 8; ++k) for (int ept : {4, 6}) if (!down_nv_dia_ok(dia(k, ept), nv)) { std::printf("row chunks K=%d EPT=%d\n", k, ept); ++bad; }
    for (int k = 2; k <= 7; ++k) if (!down_nv_dia_ok(box(k, 328, 1640), nv)) { std::printf("box chunks K=%d\n", k); ++bad; }
    DownPlan q = dia(3, 4); q.mode = 2;
    DownPlan t = dia(3, 4); t.lanes = 2;
    if (down_nv_dia_ok(q, nv) || down_nv_dia_ok(t, nv)) { std::printf("mode / lanes\n"); ++bad; }
  }
  if (dia_max != 40960) { std::printf("largest LDS of the row chunks %zu, expected 40960\n", dia_max); ++bad; }
  if (box_max != 131072) { std::printf("largest LDS of the boxes walked %zu, expected 131072 (2048 rows, NV 4)\n", box_max); ++bad; }
  std::printf("cases=%ld admitted=%ld dia=%ld box=%ld bad=%d\n", cases, admitted, admitted_dia, admitted_box, bad);
  return bad ? 1 : 0;
}
"""


def build_and_run(tmp_path, flags=()):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to compile down_plan.hpp")
    src = tmp_path / "down_plan_dia_check.cpp"
    exe = tmp_path / "down_plan_dia_check"
    src.write_text(PROGRAM)
    inc = os.path.join(ROOT, "ngsamg_amd", "csrc", "device")
    cc = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *flags, "-I", inc, "-o", str(exe), str(src)],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    return subprocess.run([str(exe)], capture_output=True, text=True)


def test_down_nv_dia_rule_host_program(tmp_path):
    run = build_and_run(tmp_path)
    assert run.returncode == 0, run.stdout + run.stderr
    last = run.stdout.strip().splitlines()[-1]
    fields = dict(f.split("=") for f in last.split())
    # 5 families x 3 modes x 3 sizes x 3 lane counts x 5 EPTs x 8 diagonal counts x 6 boxes x 5 widths x on / off
    assert int(fields["cases"]) == 5 * 3 * 3 * 3 * 5 * 8 * 6 * 5 * 2 and int(fields["bad"]) == 0, run.stdout
    # row chunks: 6 of the diagonal counts walked (1, 2, 3, 5, 7, 8) x 2 EPTs x 6 boxes (ignored) x 2 widths
    assert int(fields["dia"]) == 6 * 2 * 6 * 2, run.stdout
    # box chunks: 4 of the diagonal counts walked (2, 3, 5, 7) x 5 EPTs (ignored) x the boxes that fit: 4 at both widths,
    # 6000 x 100 at none (8 * 2 * 6000 * 2 = 192000), 2048 x 20000 at none (8 * (4096 + 20000) = 192768)
    assert int(fields["box"]) == 4 * 5 * 4 * 2, run.stdout
    assert int(fields["admitted"]) == int(fields["dia"]) + int(fields["box"])
