"""ngsamg_amd/csrc/device/krylov_core.hpp (pcg, pcg_sr, gmres over a space) compiled by a plain C++17 host compiler and run over
a host space: vectors are std::vector<double>, sums are sequential, A is a CSR matrix read from a file, C is the inverse diagonal
or the identity.  The three bodies are the ones the device library runs over its two spaces (krylov.hpp, dist.hpp), so what is
pinned here -- recurrences, stop rules, the partial-cycle exit of GMRES, maxit = 0, a null history -- is pinned for them too.
The same program is built once more with -fsanitize=address,undefined and run on the same inputs."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

from tests.krylov_cases import numpy_pcg, rel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include "krylov_core.hpp"
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

struct HostSpace {
  using V = std::vector<double>;
  using Vec = V*;
  using CVec = const V*;
  int n = 0;
  std::vector<int> rowptr, col;
  V val, dinv;
  bool jacobi = true;                        // C = inverse diagonal, else the identity
  V res, op, wk[3];
  std::vector<V> B;                          // GMRES basis
  double sc[64] = {};

  void begin(amgx::Form f, int restart) {
    res.assign(n, 0.0); op.assign(n, 0.0);
    for (V& v : wk) v.assign(n, 0.0);
    if (f == amgx::Form::GMRES) B.assign(std::max(1, restart) + 1, V(n, 0.0));
  }
  Vec residual_vec() { return &res; }
  Vec operand() { return &op; }
  Vec work(int k) { return &wk[k]; }
  Vec basis(int j) { return &B[j]; }

  void mult(CVec v, Vec y) {
    V out(n);
    for (int i = 0; i < n; ++i) { double s = 0.0; for (int k = rowptr[i]; k < rowptr[i + 1]; ++k) s += val[k] * (*v)[col[k]]; out[i] = s; }
    *y = out;
  }
  void residual(CVec x, CVec b, Vec r) { V ax(n); mult(x, &ax); for (int i = 0; i < n; ++i) (*r)[i] = (*b)[i] - ax[i]; }
  void precond(CVec r, Vec z, bool use_pre) {
    if (!use_pre || !jacobi) { copy(z, r); return; }
    for (int i = 0; i < n; ++i) (*z)[i] = dinv[i] * (*r)[i];
  }
  double sum(CVec a, CVec b) const { double s = 0.0; for (int i = 0; i < n; ++i) s += (*a)[i] * (*b)[i]; return s; }
  void dot(CVec a, CVec b, int slot) { sc[slot] = sum(a, b); }
  void multi_dot(int m, CVec w) { for (int j = 0; j < m; ++j) sc[j] = sum(&B[j], w); }
  double read(int slot) { return sc[slot]; }
  void read(int slot0, int m, double* out) { for (int j = 0; j < m; ++j) out[j] = sc[slot0 + j]; }
  void write(int slot, double v) { sc[slot] = v; }
  void sr_reduce(CVec r, CVec u, CVec w) {
    using namespace amgx;
    const double g = sum(r, u), d = sum(w, u);
    const bool first = sc[SR_FIRST] != 0.0;
    const double beta = first ? 0.0 : g / sc[SR_GOLD];
    const double alpha = first ? g / d : g / (d - beta * g / sc[SR_ALPHA]);
    sc[SR_GNEW] = g; sc[SR_DELTA] = d; sc[SR_BETA] = beta; sc[SR_ALPHA] = alpha; sc[SR_GOLD] = g; sc[SR_FIRST] = 0.0;
  }
  void copy(Vec dst, CVec src) { if (dst != src) *dst = *src; }
  void zero(Vec a, Vec b) { a->assign(n, 0.0); b->assign(n, 0.0); }
  void scale(double alpha, CVec x, Vec y) { for (int i = 0; i < n; ++i) (*y)[i] = alpha * (*x)[i]; }
  void cg_update(int num, int den, CVec s, CVec q, Vec x, Vec d) {
    const double alpha = sc[num] / sc[den];
    for (int i = 0; i < n; ++i) { (*x)[i] += alpha * (*s)[i]; (*d)[i] -= alpha * (*q)[i]; }
  }
  void xpby(int num, int den, CVec w, Vec s) {
    const double beta = sc[num] / sc[den];
    for (int i = 0; i < n; ++i) (*s)[i] = (*w)[i] + beta * (*s)[i];
  }
  void sr_update(CVec u, CVec w, Vec p, Vec s, Vec x, Vec r) {
    const double alpha = sc[amgx::SR_ALPHA], beta = sc[amgx::SR_BETA];
    for (int i = 0; i < n; ++i) {
      const double pi = (*u)[i] + beta * (*p)[i], si = (*w)[i] + beta * (*s)[i];
      (*p)[i] = pi; (*s)[i] = si;
      (*x)[i] += alpha * pi;
      (*r)[i] -= alpha * si;
    }
  }
  void basis_update(int m, const double* c, double sign, Vec w) {
    for (int i = 0; i < n; ++i) { double acc = (*w)[i]; for (int j = 0; j < m; ++j) acc += sign * c[j] * B[j][i]; (*w)[i] = acc; }
  }
};

static double number(std::istream& in) { std::string t; in >> t; return std::strtod(t.c_str(), nullptr); }   // (hexadecimal floats too)

// input: n nnz / rowptr / col / val / nruns / per run: kind use_pre jacobi tol maxit restart null_errs, then b, then x0
// output per run: "it <count>", the maxit + 1 history entries (pre-set to -1), x; doubles as hexadecimal floats
int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::ifstream in(argv[1]);
  HostSpace S;
  int nnz = 0, nruns = 0;
  in >> S.n >> nnz;
  S.rowptr.resize(S.n + 1); S.col.resize(nnz); S.val.resize(nnz); S.dinv.assign(S.n, 0.0);
  for (int& v : S.rowptr) in >> v;
  for (int& v : S.col) in >> v;
  for (double& v : S.val) v = number(in);
  for (int i = 0; i < S.n; ++i) for (int k = S.rowptr[i]; k < S.rowptr[i + 1]; ++k) if (S.col[k] == i) S.dinv[i] = 1.0 / S.val[k];
  in >> nruns;
  for (int r = 0; r < nruns; ++r) {
    std::string kind;
    int use_pre = 0, jac = 0, maxit = 0, restart = 0, null_errs = 0;
    double tol = 0.0;
    in >> kind >> use_pre >> jac;
    tol = number(in);
    in >> maxit >> restart >> null_errs;
    std::vector<double> b(S.n), x(S.n), errs(maxit + 1, -1.0);
    for (double& v : b) v = number(in);
    for (double& v : x) v = number(in);
    if (!in) return 3;
    S.jacobi = jac != 0;
    double* e = null_errs ? nullptr : errs.data();
    int it = -1;
    if (kind == "pcg") it = amgx::pcg(S, &b, &x, tol, maxit, use_pre != 0, e);
    else if (kind == "pcg_sr") it = amgx::pcg_sr(S, &b, &x, tol, maxit, e);
    else if (kind == "gmres") it = amgx::gmres(S, &b, &x, tol, maxit, restart, use_pre != 0, e);
    else return 4;
    std::printf("it %d\n", it);
    for (double v : errs) std::printf("%a ", v);
    std::printf("\n");
    for (double v : x) std::printf("%a ", v);
    std::printf("\n");
  }
  return 0;
}
"""

TOL, MAXIT = 1e-10, 100                      # as tests/test_krylov_cpu.py runs the oracle's PCG
GMRES_MAXIT = 300
RESTARTS = (5, 12, 30)


def laplacian(nx, ny):
    def t(n):
        return sp.diags([-np.ones(n - 1), 2.0 * np.ones(n), -np.ones(n - 1)], [-1, 0, 1])
    return (sp.kron(sp.identity(ny), t(nx)) + sp.kron(t(ny), sp.identity(nx))).tocsr()


def systems():
    out = {}
    for shape in ((7, 9), (5, 13)):
        A = laplacian(*shape)
        out["lap%dx%d" % shape] = (A, np.random.default_rng(3).standard_normal(A.shape[0]))
    out["one"] = (sp.csr_matrix(np.array([[2.0]])), np.array([3.0]))
    A = laplacian(7, 9)
    out["zero_rhs"] = (A, np.zeros(A.shape[0]))
    return out


def starts(n):
    return {"cold": np.zeros(n), "guess": 10.0 * np.random.default_rng(5).standard_normal(n)}


def run_list(n):
    """(key, kind, use_pre, jacobi, tol, maxit, restart, null_errs, start)"""
    runs = []
    for st in ("cold", "guess"):
        for jac in (1, 0):
            runs.append((("pcg", jac, st), "pcg", 1, jac, TOL, MAXIT, 0, 0, st))
            for m in RESTARTS:
                runs.append((("gmres", m, jac, st), "gmres", 1, jac, TOL, GMRES_MAXIT, m, 0, st))
        runs.append((("pcg_nopre", st), "pcg", 0, 1, TOL, MAXIT, 0, 0, st))            # use_pre = false: the identity, whatever C is
        runs.append((("pcg_sr", st), "pcg_sr", 1, 1, TOL, MAXIT, 0, 0, st))
        runs.append((("gmres_cut", st), "gmres", 1, 1, 1e-30, 10, 7, 0, st))           # stopped by maxit inside its second cycle
        for kind, m in (("pcg", 0), ("pcg_sr", 0), ("gmres", 5)):
            runs.append((("maxit0", kind, st), kind, 1, 1, TOL, 0, m, 0, st))
            runs.append((("null", kind, st), kind, 1, 1, TOL, MAXIT, m, 1, st))
            runs.append((("nonnull", kind, st), kind, 1, 1, TOL, MAXIT, m, 0, st))
    return runs


def write_input(path, A, b):
    n = A.shape[0]
    x0 = starts(n)
    with open(path, "w") as f:
        f.write(f"{n} {A.nnz}\n" + " ".join(map(str, A.indptr)) + "\n" + " ".join(map(str, A.indices)) + "\n")
        f.write(" ".join(float(v).hex() for v in A.data) + "\n")
        runs = run_list(n)
        f.write(f"{len(runs)}\n")
        for _, kind, pre, jac, tol, maxit, m, null, st in runs:
            f.write(f"{kind} {pre} {jac} {tol!r} {maxit} {m} {null}\n")
            f.write(" ".join(float(v).hex() for v in b) + "\n" + " ".join(float(v).hex() for v in x0[st]) + "\n")


def parse(text, n):
    lines = text.strip().split("\n")
    runs = run_list(n)
    assert len(lines) == 3 * len(runs)
    out = {}
    for i, r in enumerate(runs):
        tag, it = lines[3 * i].split()
        assert tag == "it"
        errs = np.array([float.fromhex(t) for t in lines[3 * i + 1].split()])
        x = np.array([float.fromhex(t) for t in lines[3 * i + 2].split()])
        assert errs.size == r[5] + 1 and x.size == n
        out[r[0]] = (x, int(it), errs)
    return out


def compile_program(tmp, name, extra):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to compile krylov_core.hpp")
    src = tmp / "krylov_core_check.cpp"
    src.write_text(PROGRAM)
    exe = tmp / name
    inc = os.path.join(ROOT, "ngsamg_amd", "csrc", "device")
    cc = subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", *extra, "-I", inc, "-o", str(exe), str(src)],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    return exe


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("krylov_core")
    for name, (A, b) in systems().items():
        write_input(tmp / f"{name}.txt", A, b)
    return tmp


@pytest.fixture(scope="module")
def results(workdir):
    exe = compile_program(workdir, "krylov_core_check", ["-O1"])
    out = {}
    for name, (A, _) in systems().items():
        run = subprocess.run([str(exe), str(workdir / f"{name}.txt")], capture_output=True, text=True)
        assert run.returncode == 0, run.stdout[-2000:] + run.stderr
        out[name] = parse(run.stdout, A.shape[0])
    return out


def test_core_header_compiles_alone(tmp_path):
    """krylov_core.hpp on its own: no HIP, no other header of the library before it"""
    src = tmp_path / "alone.cpp"
    src.write_text('#include "krylov_core.hpp"\nint main() { return 0; }\n')
    inc = os.path.join(ROOT, "ngsamg_amd", "csrc", "device")
    cc = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", inc, "-o", str(tmp_path / "alone"), str(src)],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    text = open(os.path.join(inc, "krylov_core.hpp")).read()
    assert "#include <hip" not in text and "__HIPCC__" not in text


def preconditioner(A, jac):
    dinv = 1.0 / A.diagonal()
    return (lambda v: dinv * v) if jac else (lambda v: v.copy())


def scale(b, x0, xn):
    """what a solution error is measured against: the solution's norm -- but with b = 0 the solution is 0 and what a solver returns
    is its remaining error, so two correct solvers agree only relative to the error they started from, |x0 - 0|"""
    return float(np.linalg.norm(xn)) if b.any() else float(np.linalg.norm(x0))


NAMES = list(systems())
STARTS = ("cold", "guess")


@pytest.mark.parametrize("start", STARTS)
@pytest.mark.parametrize("name", NAMES)
def test_pcg_equals_numpy_pcg(results, name, start):
    """history, count and solution against the textbook recurrence: same count, whole history to 1e-9, solution to 1e-8
    (the bounds of test_oracle_pcg_with_initial_guess_equals_numpy_pcg); the entries behind the last iteration are not written"""
    A, b = systems()[name]
    x0 = starts(A.shape[0])[start]
    for key, C in ((("pcg", 1, start), preconditioner(A, 1)), (("pcg", 0, start), preconditioner(A, 0)),
                   (("pcg_nopre", start), preconditioner(A, 0))):
        x, it, errs = results[name][key]
        xn, itn, en = numpy_pcg(A, C, b, x0, TOL, MAXIT)
        print(f"{name} {key}: it {it} / {itn}, err_0 {en[0]:.3e}, last {en[-1]:.3e}, solution {rel(x, xn):.1e}")
        assert it == itn and it < MAXIT
        assert np.all(errs[it + 1:] == -1.0)
        assert np.allclose(errs[:it + 1], en, rtol=1e-9, atol=0)
        assert np.linalg.norm(x - xn) <= 1e-8 * scale(b, x0, xn)
        if name == "zero_rhs" and start == "cold":
            assert it == 0 and errs[0] == 0.0 and not x.any()
        if name == "zero_rhs" and start == "guess":
            assert 0 < it and np.linalg.norm(x) <= 1e-8 * np.linalg.norm(x0)
        if name == "one":
            assert it == 1


@pytest.mark.parametrize("start", STARTS)
@pytest.mark.parametrize("name", NAMES)
def test_single_reduction_pcg_equals_numpy_pcg(results, name, start):
    """the Chronopoulos / Gear form against the classical recurrence, as test_single_reduction_pcg_history_equals_classical holds
    the two forms together on the device: count +-1, common history to 1e-6, solution to 1e-8"""
    A, b = systems()[name]
    x0 = starts(A.shape[0])[start]
    x, it, errs = results[name][("pcg_sr", start)]
    xn, itn, en = numpy_pcg(A, preconditioner(A, 1), b, x0, TOL, MAXIT)
    print(f"{name}: it {it} / {itn}")
    assert abs(it - itn) <= 1
    k = min(it, itn)
    assert np.all(errs[it + 1:] == -1.0)
    assert np.allclose(errs[:k], en[:k], rtol=1e-6)
    assert np.linalg.norm(x - xn) <= 1e-8 * scale(b, x0, xn)


@pytest.mark.parametrize("start", STARTS)
@pytest.mark.parametrize("name", NAMES)
def test_gmres_minimises_the_preconditioned_residual(results, name, start):
    """restart 5, 12 and 30 (30 is more than these systems need: the cycle is left early and its partial update applied): err_0 and the
    last recurrence value are the true |C (b - A x)|, the history is monotone inside every cycle, the solution is PCG's -- the
    checks of test_oracle_gmres_with_initial_guess_minimises_the_preconditioned_residual"""
    A, b = systems()[name]
    n = A.shape[0]
    x0 = starts(n)[start]
    for jac in (1, 0):
        C = preconditioner(A, jac)
        xc = numpy_pcg(A, C, b, x0, TOL, MAXIT)[0]
        for m in RESTARTS:
            x, it, errs = results[name][("gmres", m, jac, start)]
            assert np.all(errs[it + 1:] == -1.0)
            errs = errs[:it + 1]
            print(f"{name} restart {m} jac {jac}: it {it}, err_0 {errs[0]:.3e}, last {errs[-1]:.3e}")
            assert it < GMRES_MAXIT and errs[-1] <= TOL * errs[0]
            assert abs(errs[0] - np.linalg.norm(C(b - A @ x0))) <= 1e-12 * errs[0]
            for c0 in range(0, max(it, 1), m):
                cyc = errs[c0:c0 + m + 1]
                assert all(e2 <= e1 * (1 + 1e-12) for e1, e2 in zip(cyc[:-1], cyc[1:]))
            assert abs(np.linalg.norm(C(b - A @ x)) - errs[-1]) <= 1e-6 * errs[0]
            assert np.linalg.norm(x - xc) <= 1e-7 * scale(b, x0, xc)
            if m == 30 and n > 1 and errs[0] > 0:
                assert 1 < it and it % m != 0              # the last cycle ended before its m-th column
        if errs[0] == 0.0:
            assert it == 0 and np.array_equal(x, x0)
    # stopped by maxit = 10 inside the second cycle of GMRES(7): the partial cycle's update is applied
    x, it, errs = results[name][("gmres_cut", start)]
    C = preconditioner(A, 1)
    if errs[0] > 0 and n > 1:
        assert it == 10 and abs(np.linalg.norm(C(b - A @ x)) - errs[10]) <= 1e-6 * errs[0]


@pytest.mark.parametrize("name", NAMES)
def test_maxit_zero_and_null_history(results, name):
    A, b = systems()[name]
    for start, x0 in starts(A.shape[0]).items():
        C = preconditioner(A, 1)
        r0 = b - A @ x0
        for kind in ("pcg", "pcg_sr"):                       # err_0 is computed, x is untouched
            x, it, errs = results[name][("maxit0", kind, start)]
            assert it == 0 and np.array_equal(x, x0)
            assert abs(errs[0] - math.sqrt(abs(C(r0) @ r0))) <= 1e-12 * errs[0]
        x, it, errs = results[name][("maxit0", "gmres", start)]   # GMRES computes err_0 inside its first cycle: nothing runs
        assert it == 0 and np.array_equal(x, x0) and errs[0] == -1.0
        for kind in ("pcg", "pcg_sr", "gmres"):              # errs = null: the same x bit for bit, the same count
            xa, ita, _ = results[name][("null", kind, start)]
            xb, itb, eb = results[name][("nonnull", kind, start)]
            assert ita == itb and np.array_equal(xa, xb)
            assert np.all(eb[:itb + 1] >= 0.0)


def test_sanitized_build_runs_clean(workdir):
    """the same stand-alone program with AddressSanitizer and UndefinedBehaviorSanitizer on every input"""
    exe = compile_program(workdir, "krylov_core_check_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    for name in NAMES:
        run = subprocess.run([str(exe), str(workdir / f"{name}.txt")], capture_output=True, text=True)
        assert run.returncode == 0, run.stderr[-4000:]
        assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr
