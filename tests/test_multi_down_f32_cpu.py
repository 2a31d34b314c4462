"""AMGX_MULTI_FUSE_DOWN_F32: the Python words, the C value, and the host-only rule of the local-window
multi-vector down launch, down_nv_lw_ok / down_nv_lw_lds_bytes (down_plan.hpp), compiled by a plain C++17 host compiler as
tests/test_down_plan_nv_cpu.py does:
  * the three worked LDS values of the rule (8 * (W * NV + (512 / lanes) * NV + EPT * 512) bytes against 160 KiB);
  * an enumeration of (family, mode, threads, lanes, EPT, NV, W): the rule admits exactly MODE 1 of the local-window family with 512
    lanes per workgroup, lanes in DownLwLanes, EPT in DownLwEpt, widths 2 and 4, under the bound;
  * down_nv_ok (AMGX_MULTI_FUSE_DOWN) and down_nv_dia_ok (AMGX_MULTI_FUSE_DOWN_DIA) keep refusing the family."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include "down_plan.hpp"
#include <cstdio>
using namespace amgx;

static constexpr DownPlan lw(int lanes, int ept, int w, int mode = 1) {
  DownPlan p{};
  p.on = true; p.family = DOWN_FAM_LW; p.mode = mode; p.threads = DOWN_THREADS; p.lanes = lanes; p.ept = ept; p.lw_max_list = w;
  return p;
}

int main() {
  if (DownPlan().lw_max_list != 0) { std::printf("the field does not default to 0\n"); return 1; }
  // ---- the worked values
  static_assert(down_nv_lw_lds_bytes(lw(2, 4, 4352), 4) == 163840 && down_nv_lw_ok(lw(2, 4, 4352), 4), "lanes 2, EPT 4, NV 4, W 4352: 160 KiB, admitted");
  static_assert(!down_nv_lw_ok(lw(2, 4, 4353), 4), "W 4353 at NV 4: refused");
  static_assert(down_nv_lw_lds_bytes(lw(2, 4, 4608), 2) == 94208 && down_nv_lw_ok(lw(2, 4, 4608), 2), "lanes 2, EPT 4, NV 2, W 4608: 92 KiB, admitted");
  if (DOWN_NV_DIA_LDS_MAX != 163840) { std::printf("the bound moved\n"); return 1; }
  // ---- the enumeration
  long n = 0, admitted = 0, over = 0;
  for (int fam = DOWN_FAM_SELL; fam <= DOWN_FAM_DIA_BOX; ++fam) for (int mode = 0; mode <= 2; ++mode) for (int threads : {256, 512, 1024})
    for (int lanes : {1, 2, 3, 4, 8}) for (int ept : {1, 2, 3, 4, 6}) for (int nv : {1, 2, 3, 4, 8}) for (int w : {0, 1, 2048, 4352, 4353, 4480, 4608, 20000}) for (int on = 0; on < 2; ++on, ++n) {
      DownPlan p = lw(lanes, ept, w, mode);
      p.family = fam; p.threads = threads; p.on = on;
      const bool shape = on && fam == DOWN_FAM_LW && mode == 1 && threads == 512 && (lanes == 2 || lanes == 4) && (ept == 2 || ept == 4) && (nv == 2 || nv == 4);
      const size_t bytes = 8 * ((size_t)w * nv + (size_t)(512 / lanes) * nv + (size_t)ept * 512);
      const bool want = shape && bytes <= 163840;
      if (shape && down_nv_lw_lds_bytes(p, nv) != bytes) { std::printf("bytes: lanes %d ept %d nv %d w %d: %zu, expected %zu\n", lanes, ept, nv, w, down_nv_lw_lds_bytes(p, nv), bytes); return 1; }
      if (down_nv_lw_ok(p, nv) != want) { std::printf("fam %d mode %d threads %d lanes %d ept %d nv %d w %d on %d: %d, expected %d\n", fam, mode, threads, lanes, ept, nv, w, on, (int)down_nv_lw_ok(p, nv), (int)want); return 1; }
      admitted += want; over += shape && !want;
      // the rules of the other two bits do not admit the family, whatever the shape
      if (fam == DOWN_FAM_LW && (down_nv_ok(p, nv) || down_nv_dia_ok(p, nv))) { std::printf("down_nv_ok / down_nv_dia_ok admit the local-window family\n"); return 1; }
    }
  if (!admitted || !over) { std::printf("a class is empty: %ld %ld\n", admitted, over); return 1; }
  // the lists the rule reads are the single-vector family's
  static_assert(contains(DownLwLanes{}, 2) && contains(DownLwLanes{}, 4) && !contains(DownLwLanes{}, 1) && !contains(DownLwLanes{}, 8), "DownLwLanes");
  static_assert(contains(DownLwEpt{}, 2) && contains(DownLwEpt{}, 4) && !contains(DownLwEpt{}, 6), "DownLwEpt");
  // a level takes the pass only if both widths fit: the longest list the family can have (LW_CAP = 4608) fits NV = 2 alone
  if (!down_nv_lw_ok(lw(2, 4, 4608), 2) || down_nv_lw_ok(lw(2, 4, 4608), 4) || !down_nv_lw_ok(lw(4, 4, 4480), 4) || down_nv_lw_ok(lw(4, 4, 4481), 4)) { std::printf("the bound at the capacity\n"); return 1; }
  std::printf("ok %ld admitted=%ld over=%ld\n", n, admitted, over);
  return 0;
}
"""


def test_local_window_rule(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to compile down_plan.hpp")
    src, exe = tmp_path / "down_lw.cpp", tmp_path / "down_lw"
    src.write_text(PROGRAM)
    cc = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "ngsamg_amd", "csrc", "device"),
                         "-o", str(exe), str(src)], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout + out.stderr
    fields = dict(f.split("=") for f in out.stdout.split()[2:])
    assert int(out.stdout.split()[1]) == 5 * 3 * 3 * 5 * 5 * 5 * 8 * 2, out.stdout
    assert int(fields["admitted"]) > 0 and int(fields["over"]) > 0, out.stdout


def test_python_words_and_values():
    from ngsamg_amd import _lib
    from ngsamg_amd._lib import NgsAMGError
    from ngsamg_amd.device import check_fuse
    assert _lib.AMGX_MULTI_FUSE_DOWN_F32 == 4096
    assert check_fuse("gs+down_f32") == 64 | 128 | 512 | 2048 | 4096 == 6848
    assert check_fuse("gs_block+down_f32") == 64 | 128 | 256 | 512 | 2048 | 4096 == 7104
    # the bit implies AMGX_MULTI_FUSE_DOWN and AMGX_MULTI_FUSE_F32: the words carry them; the Gauss-Seidel bits are the word's
    for word in ("gs", "gs_block"):
        assert check_fuse(word + "+down_f32") == check_fuse(word + "+down+f32") | _lib.AMGX_MULTI_FUSE_DOWN_F32, word
    # every other word and value is what it was
    assert [check_fuse(w) for w in (False, True, "gs", "gs_block", "down", "gs+down", "gs_block+down", "down_dia", "gs+down_dia", "gs_block+down_dia",
                                    "gs+f32", "gs_block+f32", "gs+down+f32", "gs_block+down+f32")] == \
        [0, 64, 192, 448, 576, 704, 960, 1600, 1728, 1984, 2240, 2496, 2752, 3008]
    for bad in ("f32", "+f32", "down+f32", "gs+f32+down", "gs+down_dia+f32", "GS+F32", "gs +f32", 2048, None, 1,
                "down_f32", "+down_f32", "gs+down_f32+f32", "gs+down_dia_f32", "gs+down_dia+down_f32", "GS+DOWN_F32", 4096, 6848):
        with pytest.raises(NgsAMGError, match="fuse: need True, False") as ei:
            check_fuse(bad)
        assert '"gs+f32"' in str(ei.value) and '"gs+down_f32"' in str(ei.value) and repr(bad) in str(ei.value), str(ei.value)


def test_header_declares_the_value():
    text = open(os.path.join(ROOT, "include", "amgx.h")).read()
    m = re.search(r"\bAMGX_MULTI_FUSE_DOWN_F32\s*=\s*(\d+)", text)
    assert m and int(m.group(1)) == 4096, m
    src = ('#include "amgx.h"\n_Static_assert(AMGX_MULTI_FUSE_DOWN_F32 == 4096, "value");\n'
           '_Static_assert((AMGX_MULTI_FUSE_DOWN_F32 & (AMGX_MULTI_FUSE | AMGX_MULTI_FUSE_GS | AMGX_MULTI_FUSE_GS_BLOCK | AMGX_MULTI_FUSE_DOWN | '
           'AMGX_MULTI_FUSE_DOWN_DIA | AMGX_MULTI_FUSE_F32 | AMGX_MULTI_INTERLEAVED | AMGX_PCG_SINGLE_REDUCTION | AMGX_DEVICE_PTR | AMGX_NO_GRAPH)) == 0, '
           '"a bit of its own");\n_Static_assert(AMGX_MULTI_FUSE_F32 == 2048 && AMGX_MULTI_FUSE_DOWN_DIA == 1024 && AMGX_MULTI_FUSE_DOWN == 512, "the others");\n'
           'int main(void){return 0;}\n')
    cc = subprocess.run(["gcc", "-std=c11", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c", "-"], input=src,
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
