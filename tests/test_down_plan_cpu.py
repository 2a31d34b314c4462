"""ngsamg_amd/csrc/device/down_plan.hpp (the host arithmetic of the fused down launcher) compiled by a plain C++17 host compiler
into a stand-alone program.

For every family, the workgroup sizes 256 / 512 / 1024, 1 / 2 / 4 / 8 lanes per row and 0, 1, 7, 8, 9, 16, 17 slices:
  * the expected chunk count is the smallest number of chunks that holds the slices (dia: the rows; dia-box: one chunk per box);
  * for n_int = 0, n_rows and every chunk boundary with its two neighbours: the interior and the boundary range are disjoint,
    together they are the whole range, a chunk is interior exactly when all its rows lie below n_int (so a chunk that straddles
    n_int is a boundary chunk), and PART_ALL covers everything;
  * an unsplittable plan (diagonal image, box chunks, compact chunks) covers everything under PART_ALL and refuses the parts.
unit_range is the function Handle::product uses for its slices and windows, so the same properties hold there.
The program is built twice: plainly, and with AddressSanitizer + UndefinedBehaviorSanitizer (it runs on its own, outside Python)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include "down_plan.hpp"
#include <cstdio>
#include <set>

using namespace amgx;

int main() {
  int bad = 0;
  long cases = 0;
  const int families[] = {DOWN_FAM_SELL, DOWN_FAM_WIN, DOWN_FAM_LW, DOWN_FAM_DIA, DOWN_FAM_DIA_BOX};
  const int sizes[] = {256, 512, 1024}, lanes_of[] = {1, 2, 4, 8};
  const int64_t slice_counts[] = {0, 1, 7, 8, 9, 16, 17};
  for (int fam : families) for (int threads : sizes) for (int lanes : lanes_of) for (int64_t slices : slice_counts) for (int compact = 0; compact < 2; ++compact) {
    auto fail = [&](const char* what, int64_t n_int) {
      std::printf("family=%d threads=%d lanes=%d slices=%lld compact=%d n_int=%lld: %s\n", fam, threads, lanes, (long long)slices, compact, (long long)n_int, what);
      ++bad;
    };
    const int64_t u = down_rows_per_chunk(threads, lanes);
    if (u * lanes != threads || down_slices_per_chunk(threads) * DOWN_SLICE != threads) fail("rows / slices per chunk", -1);
    // the rows behind `slices` slices of 64 lanes: the last slice may be ragged
    const int64_t full_rows = slices * DOWN_SLICE / lanes;
    const int64_t row_counts[] = {full_rows, full_rows > 0 ? full_rows - DOWN_SLICE / lanes + 1 : 0};
    for (int64_t n_rows : row_counts) {
      // ---- chunk count
      int64_t n;
      if (fam == DOWN_FAM_DIA_BOX) {
        n = down_expected_chunks(fam, slices, threads, lanes);
        if (n != slices) fail("dia-box: one chunk per box", -1);
      } else {
        n = down_expected_chunks(fam, fam == DOWN_FAM_DIA ? n_rows : slices, threads, lanes);
        const int64_t lanes_used = fam == DOWN_FAM_DIA ? n_rows * lanes : slices * DOWN_SLICE;      // (lanes the image occupies, padded to slices)
        const int64_t padded = (lanes_used + DOWN_SLICE - 1) / DOWN_SLICE * DOWN_SLICE;
        if (n < 0 || n * threads < padded || (n > 0 && (n - 1) * threads >= padded)) fail("chunk count is not the smallest that holds the slices", -1);
      }
      // ---- ranges
      DownPlan p;
      p.on = true; p.family = fam; p.threads = threads; p.lanes = lanes; p.n_chunks = (int)n; p.unit_rows = u;
      p.splittable = down_splittable(fam, compact != 0);
      const bool expect_split = !compact && (fam == DOWN_FAM_SELL || fam == DOWN_FAM_WIN || fam == DOWN_FAM_LW);
      if (p.splittable != expect_split) fail("splittable rule", -1);
      std::set<int64_t> points = {0, n_rows};
      for (int64_t c = 0; c <= n; ++c) for (int64_t d = -1; d <= 1; ++d) if (c * u + d >= 0 && c * u + d <= n_rows) points.insert(c * u + d);
      for (int64_t n_int : points) {
        ++cases;
        int64_t a0 = -7, b0 = -7, a1 = -7, b1 = -7, a2 = -7, b2 = -7;
        if (!down_chunk_range(p, Span{PART_ALL, n_int}, a0, b0) || a0 != 0 || b0 != n) fail("PART_ALL is the whole range", n_int);
        const bool ri = down_chunk_range(p, Span{PART_INT, n_int}, a1, b1), rb = down_chunk_range(p, Span{PART_BND, n_int}, a2, b2);
        if (!p.splittable) {
          if (ri || rb || a1 != -7 || b2 != -7) fail("an unsplittable plan refuses the parts and leaves the range alone", n_int);
          continue;
        }
        if (!ri || !rb) { fail("a splittable plan refused a part", n_int); continue; }
        if (a1 != 0 || b1 != a2 || b2 != n || b1 < a1 || b2 < a2) fail("interior and boundary are not disjoint ranges that make up the whole", n_int);
        for (int64_t c = 0; c < n; ++c) {
          const bool interior = (c + 1) * u <= n_int;              // all rows of the chunk lie below n_int
          const bool in_int = c >= a1 && c < b1, in_bnd = c >= a2 && c < b2;
          if (in_int == in_bnd || in_int != interior) { fail("a chunk is in the wrong part", n_int); break; }
        }
        // the same through unit_range itself, as Handle::product calls it
        int64_t a, b;
        unit_range(Span{PART_INT, n_int}, u, n, a, b);
        if (a != a1 || b != b1) fail("unit_range differs from down_chunk_range", n_int);
      }
    }
  }
  static_assert(down_sell_lanes_ok(1) && down_sell_lanes_ok(8) && !down_sell_lanes_ok(3) && !down_sell_lanes_ok(16), "lanes of the sell family");
  std::printf("cases=%ld bad=%d\n", cases, bad);
  return bad ? 1 : 0;
}
"""


def build_and_run(tmp_path, flags=()):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to compile down_plan.hpp")
    src = tmp_path / "down_plan_check.cpp"
    exe = tmp_path / "down_plan_check"
    src.write_text(PROGRAM)
    inc = os.path.join(ROOT, "ngsamg_amd", "csrc", "device")
    cc = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *flags, "-I", inc, "-o", str(exe), str(src)],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    return subprocess.run([str(exe)], capture_output=True, text=True)


# the second build: AddressSanitizer and UndefinedBehaviorSanitizer, runtimes linked statically into the stand-alone program
SANITIZE = ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan")


@pytest.mark.parametrize("flags", [(), SANITIZE], ids=["plain", "asan-ubsan"])
def test_down_plan_host_program(tmp_path, flags):
    run = build_and_run(tmp_path, flags)
    assert run.returncode == 0, run.stdout + run.stderr
    last = run.stdout.strip().splitlines()[-1]
    assert last.endswith("bad=0") and int(last.split()[0].split("=")[1]) > 5000, run.stdout
