"""ngsamg_amd/csrc/device/knobs.hpp, the one place that reads the environment switches of the device library.

Host program: knobs.hpp is host code, so a stand-alone program (its own main, nothing preloaded) includes it, sets the environment
from its arguments (NAME=VALUE), calls Knobs::from_env() and prints every field.  It is compiled with -Wall -Wextra -Werror and once
more with -fsanitize=address,undefined.  Checked: the documented defaults under an empty environment, every boolean switch on its
own (its field turns on, no other boolean does), AMGX_FUSED_BLOCK outside its list, AMGX_DIA_BOX_SHAPE, the clamp of
AMGX_BSELL_XMODE, and AMGX_SELL_LONG_ROW_LANES / AMGX_SELL_MAX_LANES: the SELL kernels exist for G in {1, 2, 4, 8, 16} only
(R = WAVE / G rows per wave), so from_env maps every value to the next lower one of them.

Completeness: every AMGX_* name of knobs.hpp occurs in at least one other file under tests/, so that a switch cannot be added
without a test that names it.  EXEMPT lists the log-only switches."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOBS = os.path.join(ROOT, "ngsamg_amd", "csrc", "device", "knobs.hpp")

# switches without a test: log-only ones, nothing else (name -> reason)
EXEMPT = {"AMGX_SETUP_LOG": "prints the wall-clock times of amgx_create on stderr, selects no code path"}


def _text():
    with open(KNOBS) as f:
        return f.read()


def _bool_switches():
    """(field, name) of every switch that from_env reads with on(name)"""
    return re.findall(r"k\.(\w+) = on\(\"(AMGX_[A-Z0-9_]+)\"\);", _text())


# fields that are not plain on / off switches: (field, printf format, cast)
OTHER_FIELDS = [("setup_threads", "%d", "int"), ("dev_images_min_rows", "%lld", "long long"), ("sell_max_lanes", "%d", "int"),
                ("sell_long_row_lanes", "%d", "int"), ("bsell_xmode", "%d", "int"), ("xcd", "%d", "int"),
                ("dia_min_rows", "%lld", "long long"), ("dia_max_fill", "%.17g", "double"), ("dia_box_min_rows", "%lld", "long long"),
                ("dia_box_yc", "%d", "int"), ("dia_box_zc", "%d", "int"), ("lw_min_rows", "%lld", "long long"),
                ("lw_test_cap", "%lld", "long long"), ("fused_block", "%d", "int"), ("fused_ept_max", "%d", "int"),
                ("compact_chunks_min_rows", "%lld", "long long"), ("restrict_min_rows", "%lld", "long long"),
                ("q_max_pad", "%.17g", "double"), ("bgs_bsell_min", "%lld", "long long"), ("dense_max", "%lld", "long long"),
                ("coarse_dense_max", "%lld", "long long"), ("dist_graph", "%d", "int"), ("dist_force_allgather", "%d", "int")]

# the defaults as the comments of the struct document them (setup_threads: min(cores, 32), fused_block: DOWN_THREADS -- below)
DEFAULTS = {"dev_images_min_rows": 65536, "sell_max_lanes": 0, "sell_long_row_lanes": 1, "bsell_xmode": 0, "xcd": 1,
            "dia_min_rows": 2000000, "dia_max_fill": 1.05, "dia_box_min_rows": 200000, "dia_box_yc": 0, "dia_box_zc": 0,
            "lw_min_rows": 100000, "lw_test_cap": 0, "fused_ept_max": 2**31 - 1, "compact_chunks_min_rows": 200000,
            "restrict_min_rows": 2**63 - 1, "q_max_pad": 1.6, "bgs_bsell_min": 4096, "dense_max": 8192, "coarse_dense_max": 16384,
            "dist_graph": 1, "dist_force_allgather": 0}


def _program():
    lines = ['#include "knobs.hpp"', "#include <cstdio>", "#include <cstdlib>", "#include <cstring>", "#include <string>", "#include <vector>", "",
             "static void report() {",
             "  const amgx::Knobs k = amgx::Knobs::from_env();"]
    for f, _ in _bool_switches():
        lines.append(f'  std::printf("{f}=%d\\n", (int)k.{f});')
    for f, fmt, cast in OTHER_FIELDS:
        lines.append(f'  std::printf("{f}={fmt}\\n", ({cast})k.{f});')
    lines += ['  std::printf("DOWN_THREADS=%d\\n==\\n", (int)amgx::DOWN_THREADS);', "}", "",
              "// arguments: groups of NAME=VALUE closed by --; every group is one environment, reported and taken back",
              "int main(int argc, char** argv) {",
              "  std::vector<std::string> set;",
              "  for (int i = 1; i < argc; ++i) {",
              '    if (std::strcmp(argv[i], "--") == 0) {',
              "      report();",
              "      for (const std::string& n : set) unsetenv(n.c_str());",
              "      set.clear();",
              "      continue;",
              "    }",
              "    const char* eq = std::strchr(argv[i], '=');",
              '    if (!eq) { std::printf("bad argument %s\\n", argv[i]); return 2; }',
              "    set.emplace_back(argv[i], eq - argv[i]);",
              "    if (setenv(set.back().c_str(), eq + 1, 1) != 0) return 2;",
              "  }",
              "  return 0;", "}", ""]
    return "\n".join(lines)


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def knobs_exe(request, tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to compile knobs.hpp as host code")
    d = tmp_path_factory.mktemp("knobs_" + request.param)
    src, exe = d / "knobs_check.cpp", d / "knobs_check"
    src.write_text(_program())
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-g"] if request.param == "sanitized" else []
    cc = subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", *extra, "-I", os.path.dirname(KNOBS), "-o", str(exe), str(src)],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    return str(exe)


def _run_many(exe, envs):
    """the fields of Knobs::from_env() under each of the environments `envs` (dicts; nothing else named AMGX_* is set), one process"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("AMGX_")}
    args = []
    for kw in envs:
        args += [f"{k}={v}" for k, v in kw.items()] + ["--"]
    run = subprocess.run([exe] + args, capture_output=True, text=True, env=env)
    assert run.returncode == 0, run.stdout + run.stderr
    outs = []
    for block in run.stdout.split("==\n")[:-1]:
        out = {}
        for ln in block.split():
            k, v = ln.split("=")
            out[k] = float(v) if k in ("dia_max_fill", "q_max_pad") else int(v)
        outs.append(out)
    assert len(outs) == len(envs)
    return outs


def _run(exe, **kw):
    return _run_many(exe, [kw])[0]


def test_struct_fields_are_all_printed():
    """the program prints every field of Knobs: a new field must be added to OTHER_FIELDS or be read with on()"""
    txt = _text()
    body = txt[txt.index("struct Knobs {"):txt.index("static Knobs from_env()")]
    body = re.sub(r"//.*", "", body)
    fields = set()
    for decl in re.findall(r"\b(?:bool|int|int64_t|double)\s+([^;]+);", body):
        fields |= {re.match(r"\s*(\w+)", part).group(1) for part in decl.split(",")}
    printed = {f for f, _ in _bool_switches()} | {f for f, _, _ in OTHER_FIELDS}
    assert fields == printed, fields ^ printed


def test_defaults(knobs_exe):
    k = _run(knobs_exe)
    for f, _ in _bool_switches():
        assert k[f] == 0, f
    for f, v in DEFAULTS.items():
        assert k[f] == v, (f, k[f], v)
    assert k["fused_block"] == k["DOWN_THREADS"] and k["DOWN_THREADS"] in (256, 512, 1024)
    assert 1 <= k["setup_threads"] <= 32


def test_every_boolean_switch_turns_on_alone(knobs_exe):
    sw = _bool_switches()
    assert len(sw) >= 40 and len({n for _, n in sw}) == len(sw) == len({f for f, _ in sw})
    for (field, name), k in zip(sw, _run_many(knobs_exe, [{name: "1"} for _, name in sw])):
        on = [f for f, _ in sw if k[f]]
        assert on == [field], (name, on)
        if name != "AMGX_LW_TEST_CAP":           # (the one name that also carries a value)
            assert {f: k[f] for f in DEFAULTS} == DEFAULTS, name


def test_integer_switches(knobs_exe):
    assert _run(knobs_exe, AMGX_SETUP_THREADS="3")["setup_threads"] == 3
    assert _run(knobs_exe, AMGX_SETUP_THREADS="0")["setup_threads"] == 1
    assert _run(knobs_exe, AMGX_SETUP_THREADS="-4")["setup_threads"] == 1
    d = _run(knobs_exe)["DOWN_THREADS"]
    for v, want in ((256, 256), (512, 512), (1024, 1024), (300, d), (0, d), (-256, d), (2048, d)):
        assert _run(knobs_exe, AMGX_FUSED_BLOCK=str(v))["fused_block"] == want, v
    assert _run(knobs_exe, AMGX_FUSED_BLOCK="abc")["fused_block"] == d
    for v, want in ((-1, 0), (0, 0), (1, 1), (3, 3), (5, 5), (6, 5), (99, 5)):
        assert _run(knobs_exe, AMGX_BSELL_XMODE=str(v))["bsell_xmode"] == want, v
    assert _run(knobs_exe, AMGX_FUSED_EPT_MAX="0")["fused_ept_max"] == 0
    assert _run(knobs_exe, AMGX_COARSE_DENSE_MAX="39")["coarse_dense_max"] == 39
    assert _run(knobs_exe, AMGX_DENSE_MAX="-5")["dense_max"] == 0
    k = _run(knobs_exe, AMGX_LW_TEST_CAP="600")
    assert k["lw_test_cap_on"] == 1 and k["lw_test_cap"] == 600
    assert _run(knobs_exe, AMGX_DIST_GRAPH="0")["dist_graph"] == 0 and _run(knobs_exe, AMGX_DIST_GRAPH="1")["dist_graph"] == 1
    assert _run(knobs_exe, AMGX_DIST_FORCE_ALLGATHER="1")["dist_force_allgather"] == 1
    assert _run(knobs_exe, AMGX_DIST_FORCE_ALLGATHER="pad")["dist_force_allgather"] == 2
    assert _run(knobs_exe, AMGX_DIA_MAX_FILL="0.5")["dia_max_fill"] == 1.0
    assert _run(knobs_exe, AMGX_Q_MAX_PAD="2.5")["q_max_pad"] == 2.5


@pytest.mark.parametrize("text,want", [("4x2", (4, 2)), ("16x1", (16, 1)), ("1x1", (1, 1)), ("4", (0, 0)), ("4x", (0, 0)), ("x4", (0, 0)),
                                       ("0x4", (0, 0)), ("4x0", (0, 0)), ("-2x4", (0, 0)), ("", (0, 0)), ("axb", (0, 0))])
def test_dia_box_shape(knobs_exe, text, want):
    """YxZ with both positive, anything else keeps the default (0, 0 = chosen by the dimension)"""
    k = _run(knobs_exe, AMGX_DIA_BOX_SHAPE=text)
    assert (k["dia_box_yc"], k["dia_box_zc"]) == want


@pytest.mark.parametrize("name,field", [("AMGX_SELL_LONG_ROW_LANES", "sell_long_row_lanes"), ("AMGX_SELL_MAX_LANES", "sell_max_lanes")])
def test_lanes_per_row_are_a_power_of_two_up_to_16(knobs_exe, name, field):
    """SELL kernels exist for G in {1, 2, 4, 8, 16}: every value is rounded down to one of them (3 gave G = 3 and R = 64 / 3 rows per
    wave before)"""
    values = list(range(-2, 40)) + [63, 64, 100, 1 << 20, 2**31 - 1]
    for v, k in zip(values, _run_many(knobs_exe, [{name: str(v)} for v in values])):
        want = 1
        while want < 16 and 2 * want <= v:
            want *= 2
        assert k[field] == want, v
    assert _run(knobs_exe, **{name: "junk"})[field] == 1


def _names():
    return sorted(set(re.findall(r"\"(AMGX_[A-Z0-9_]+)\"", _text())))


def untested_switches(tests_dir):
    """the names of knobs.hpp that no file under tests_dir other than this one holds and EXEMPT does not list"""
    texts = []
    for base, _, files in os.walk(tests_dir):
        for f in sorted(files):
            if f.endswith(".py") and f != os.path.basename(__file__):
                with open(os.path.join(base, f), errors="replace") as fh:
                    texts.append(fh.read())
    return [n for n in _names() if n not in EXEMPT and not any(re.search(r"\b" + n + r"\b", t) for t in texts)]


def test_every_switch_is_named_by_a_test():
    names = _names()
    assert len(names) >= 60
    assert len(EXEMPT) <= 2 and all(n in names for n in EXEMPT) and all(r.strip() for r in EXEMPT.values())
    assert untested_switches(os.path.join(ROOT, "tests")) == []
