"""The host part of ngsamg_amd/csrc/device/launch.hpp (dispatch<V0, V1, ...>(value, f)) compiled by a plain C++17 host compiler:
every listed value reaches its own constant exactly once, an unlisted value returns false and calls nothing, and the written-out
fallback form `if (!dispatch<...>(v, run)) run(Int<F>{})` reaches the fallback constant.  The named form -- IntList<...>,
dispatch(list, value, f), contains(list, value) -- behaves the same, and contains() agrees with dispatch() on every value in -1 .. 70
for the three block-shape lists of the product launcher (key = 10 * br + bc).  The host part of the file is all this program
sees, so those lists are written out here as Handle (amgx.hip) names them.  The value lists of the fused down kernels live in the
host-only down_plan.hpp and are checked as the launcher and the builders use them: contains() and dispatch() agree on every value
in -1 .. 1100, each list holds exactly the values DESIGN.md 5.2 states, and values() yields them in their order."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include "launch.hpp"
#include "down_plan.hpp"
#include <cstdio>
#include <algorithm>
#include <initializer_list>
#include <map>
#include <type_traits>

template <int V> struct Tag { static constexpr int value = V; };   // the constant must be usable as a template argument

int main() {
  std::map<int, int> calls;                  // constant -> number of calls
  auto run = [&](auto G) {
    static_assert(std::is_same<decltype(G), amgx::Int<G()>>::value, "f receives std::integral_constant<int, Vi>");
    calls[Tag<G()>::value]++;
  };
  int bad = 0;
  const int listed[] = {1, 2, 4, 8};
  for (int v : listed) {
    calls.clear();
    if (!amgx::dispatch<1, 2, 4, 8>(v, run)) { std::printf("listed value %d: returned false\n", v); ++bad; }
    if (calls.size() != 1 || calls[v] != 1) { std::printf("listed value %d: wrong calls\n", v); ++bad; }
  }
  const int unlisted[] = {0, 3, 16, -1, 64};
  for (int v : unlisted) {
    calls.clear();
    if (amgx::dispatch<1, 2, 4, 8>(v, run)) { std::printf("unlisted value %d: returned true\n", v); ++bad; }
    if (!calls.empty()) { std::printf("unlisted value %d: something was called\n", v); ++bad; }
  }
  for (int v : unlisted) {                   // the fallback form of the SELL families: any other lane count -> 16
    calls.clear();
    if (!amgx::dispatch<1, 2, 4, 8>(v, run)) run(amgx::Int<16>{});
    if (calls.size() != 1 || calls[16] != 1) { std::printf("fallback for %d: wrong calls\n", v); ++bad; }
  }
  for (int v : listed) {                     // ... and a listed value does not take it
    calls.clear();
    if (!amgx::dispatch<1, 2, 4, 8>(v, run)) run(amgx::Int<16>{});
    if (calls.size() != 1 || calls[v] != 1) { std::printf("fallback form, listed value %d: wrong calls\n", v); ++bad; }
  }
  calls.clear();                             // an empty list matches nothing
  if (amgx::dispatch<>(1, run) || !calls.empty()) { std::printf("empty list matched\n"); ++bad; }
  // ---- the named form
  using Lanes = amgx::IntList<1, 2, 4, 8>;
  for (int v : listed) {
    calls.clear();
    if (!amgx::dispatch(Lanes{}, v, run)) { std::printf("named list, listed value %d: returned false\n", v); ++bad; }
    if (calls.size() != 1 || calls[v] != 1) { std::printf("named list, listed value %d: wrong calls\n", v); ++bad; }
    if (!amgx::contains(Lanes{}, v)) { std::printf("contains: listed value %d is missing\n", v); ++bad; }
  }
  for (int v : unlisted) {
    calls.clear();
    if (amgx::dispatch(Lanes{}, v, run)) { std::printf("named list, unlisted value %d: returned true\n", v); ++bad; }
    if (!calls.empty()) { std::printf("named list, unlisted value %d: something was called\n", v); ++bad; }
    if (amgx::contains(Lanes{}, v)) { std::printf("contains: unlisted value %d\n", v); ++bad; }
  }
  calls.clear();
  if (amgx::dispatch(amgx::IntList<>{}, 1, run) || !calls.empty() || amgx::contains(amgx::IntList<>{}, 1)) { std::printf("empty named list matched\n"); ++bad; }
  static_assert(amgx::contains(amgx::IntList<22, 33, 66>{}, 33) && !amgx::contains(amgx::IntList<22, 33, 66>{}, 36), "contains is a constant expression");
  auto agree = [&](auto list, int n_listed, int hi = 70) {
    int hits = 0;
    for (int v = -1; v <= hi; ++v) {
      calls.clear();
      const bool d = amgx::dispatch(list, v, run);
      if (d != amgx::contains(list, v)) { std::printf("contains and dispatch differ on %d\n", v); ++bad; }
      if (d && (calls.size() != 1 || calls[v] != 1)) { std::printf("shape list, value %d: wrong calls\n", v); ++bad; }
      if (!d && !calls.empty()) { std::printf("shape list, value %d: something was called\n", v); ++bad; }
      hits += d;
    }
    if (hits != n_listed) { std::printf("shape list: %d values matched, %d listed\n", hits, n_listed); ++bad; }
  };
  agree(amgx::IntList<22, 33, 66>{}, 3);                                             // square shapes
  agree(amgx::IntList<22, 33, 66, 36, 63, 23, 32>{}, 7);                             // row-lane / multi-vector kernels
  agree(amgx::IntList<22, 33, 66, 36, 63, 23, 32, 13, 31, 16, 61, 12, 21>{}, 13);    // vector form
  // ---- the lists of the fused down kernels (down_plan.hpp): the values, and contains() == dispatch() on -1 .. 1100
  auto holds = [&](auto list, std::initializer_list<int> want, const char* name) {
    agree(list, (int)want.size(), 1100);
    const auto got = amgx::values(list);
    if (got.size() != want.size() || !std::equal(got.begin(), got.end(), want.begin())) { std::printf("%s: other values than stated\n", name); ++bad; }
  };
  holds(amgx::DownEpt{}, {4, 6}, "DownEpt");
  holds(amgx::DownLwEpt{}, {2, 4}, "DownLwEpt");
  holds(amgx::DownLwLanes{}, {2, 4}, "DownLwLanes");
  holds(amgx::DownSellLanes{}, {2, 4, 8}, "DownSellLanes");
  holds(amgx::DownSizes{}, {256, 512, 1024}, "DownSizes");
  holds(amgx::DiaDiags{}, {1, 2, 3, 4, 5, 6, 7, 8}, "DiaDiags");
  holds(amgx::DiaBoxDiags{}, {2, 3, 4, 5, 6, 7}, "DiaBoxDiags");
  if (amgx::DOWN_MULTI_EPT != 4 || !amgx::contains(amgx::DownEpt{}, amgx::DOWN_MULTI_EPT) || !amgx::contains(amgx::DownSizes{}, amgx::DOWN_THREADS)) {
    std::printf("DOWN_MULTI_EPT / DOWN_THREADS are not values of their lists\n");
    ++bad;
  }
  if (amgx::values(amgx::IntList<>{}).size() != 0) { std::printf("values of the empty list\n"); ++bad; }
  std::printf("bad=%d\n", bad);
  return bad ? 1 : 0;
}
"""


def test_dispatch_host_program(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to compile the host part of launch.hpp")
    src = tmp_path / "dispatch_check.cpp"
    exe = tmp_path / "dispatch_check"
    src.write_text(PROGRAM)
    inc = os.path.join(ROOT, "ngsamg_amd", "csrc", "device")
    cc = subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", inc, "-o", str(exe), str(src)],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip().endswith("bad=0")


def test_every_launch_goes_through_launch():
    """the launch macro occurs once in the native sources, inside launch() (launch.hpp), so that every kernel launch
    is followed by its own error check"""
    hits = []
    for base, _, files in os.walk(os.path.join(ROOT, "ngsamg_amd", "csrc")):
        for f in sorted(files):
            with open(os.path.join(base, f), errors="replace") as fh:
                hits += [(f, i + 1) for i, ln in enumerate(fh) if "hipLaunchKernelGGL" in ln]
    assert len(hits) == 1 and hits[0][0] == "launch.hpp", hits
