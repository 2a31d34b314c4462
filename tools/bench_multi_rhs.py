#!/usr/bin/env python3
"""k right-hand sides: k single-vector calls against one multi-vector call, same handle, same process, alternating.

    python tools/bench_multi_rhs.py [nv] [--k 1,2,4,8] [--rounds 5] [--reps 30] [--pcg-reps 30] [--out FILE] [--commit ID]
                                    [--smoother jacobi|cheby|gs] [--degree D] [--config cfg2|cfg3|cfg5]

Builds the cfg-2 hierarchy as tools/ab_cycle.py does (fem.poisson_fast((nv,)*3), nv = 215, Jacobi) and times, with device vectors and
graph replay on one stream, per k and per round
  (a) k calls of amgx_apply on k vector pairs            (b) one amgx_apply_multi of width k (interleaved, used in place)
  (b') the same with column-major arguments (one transposition in, one out)
and the same for amgx_pcg x k against amgx_pcg_multi (tol 1e-8).  Cross-run numbers differ by several per cent between boxes and
processes, so the only yardstick is (a) of the same round.  Before any time is printed every column of (b) is compared
with (a): 1e-12 relative for the cycle, 1e-8 for the PCG solutions.  Needs a GPU.

--smoother cheby (with --degree) and --config cfg3 | cfg5 (elasticity without / with rotations, nv = 126, built as tools/bench_cheby.py
does) select handles that are fused only under AMGX_MULTI_FUSE: (b), (b') and the multi-vector PCG then carry
fuse=True, (a) stays k calls of amgx_apply / amgx_pcg on the same handle; the result goes to profiles/r14/.

--smoother gs (with --config cfg2): the library's default smoother, Gauss-Seidel in the block-hybrid form ("hgs" levels), which fuses
only under AMGX_MULTI_FUSE_GS: (b), (b') and the multi-vector PCG carry fuse="gs"; the result goes to profiles/r21/.
--smoother gs with --config cfg3 | cfg5: Gauss-Seidel on the 3x3 / 6x6 levels (block-coloured on level 0, hybrid-block below), fused
only under AMGX_MULTI_FUSE_GS_BLOCK: the calls carry fuse="gs_block"; the result goes to profiles/r22/.

--down (with any of the above; --mat-prec single for the float images of a Chebyshev handle; --tag NAME for a run under switches such
as AMGX_NO_DIA=1 AMGX_NO_LW=1): a third call per round, (d) = (b) with AMGX_MULTI_FUSE_DOWN as well, and the same for
amgx_pcg_multi.  The yardstick of (d) is (b) of the same round; every line prints multi_level_plan of the smoothed levels; the result
goes to profiles/r24/.

--dia (with --down): one more call per round, (e) = (b) with AMGX_MULTI_FUSE_DOWN_DIA as well (fuse="down_dia"), and
the same for amgx_pcg_multi.  The yardstick of (e) is (b) of the same round, as for (d); every line prints multi_level_plan of the
smoothed levels under both words; the result goes to profiles/r25/.

--mat-prec single_gs_all (with --smoother gs --config cfg2) / single_gs (with --smoother gs --config cfg3 | cfg5): the handle with
single-precision Gauss-Seidel images, fused only under AMGX_MULTI_FUSE_F32 as well.  Per round (a) k single
applications on it, (b) one multi call with fuse="gs+f32" / "gs_block+f32", (c) the same call without "+f32" (the column loop), (d) the
fused call on a double handle created in the same process; the same for amgx_pcg_multi with the iteration counts of each.  Before any
time counts, (b) equals (a) to 1e-12 and (c) equals (a) bit for bit.  The result goes to profiles/r30/.

--down-f32 (with --smoother gs --config cfg2 --mat-prec single_gs_all): two more calls per round on the single-precision handle, (e) =
(b) with AMGX_MULTI_FUSE_DOWN as well (fuse="gs+down+f32": the levels keep the literal stages) and (f) = the call with
AMGX_MULTI_FUSE_DOWN_F32 (fuse="gs+down_f32"), alternating with (a) .. (d) in the same process; the same for
amgx_pcg_multi.  The yardstick of (f) is (b) of the same round, and (d) stands beside it.  Every line prints multi_level_plan per level
under the new word; the columns of (e) and (f) are compared with (a) before any time counts.  Per level 0 .. 2 the down stage alone is
timed through DownMulti (the column loop, "gs+down+f32", "gs+down_f32").  The result goes to profiles/r31/."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _commit():
    try:
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        return "unknown"


def _stats(ts):
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "rounds_ms": ts}


def _f32(args, H, p, kw, fuse, ks, nv):
    """--mat-prec single_gs_all | single_gs: per alternating round, in one process, (a) k single applications on the
    single-precision handle, (b) one multi call on it with the "+f32" word, (c) the same call without "+f32" (the column loop), (d) the
    fused call on a double handle; and the same for amgx_pcg_multi with iteration counts"""
    import numpy as np
    import torch
    from ngsamg_amd.device import DeviceAMGMatrix
    from ngsamg_amd.krylov import NativeCGSolver
    single = DeviceAMGMatrix(H, device=0, mat_prec=args.mat_prec, **kw)
    double = DeviceAMGMatrix(H, device=0, **kw)
    word = fuse + "+f32"
    d32 = args.down_f32
    word_e, word_f = fuse + "+down+f32", fuse + "+down_f32"
    extra = "ef" if d32 else ""
    plan, old = single.multi_plan(4, fuse=word), single.multi_plan(4, fuse=fuse)
    if plan["fused"] != 1 or old["fused"] != 0 or double.multi_plan(4, fuse=fuse)["fused"] != 1:
        sys.exit(f"bench_multi_rhs: plans are not (fused, column loop, fused): {plan} {old}")
    n = p.n * p.bs
    pfree = np.repeat(p.free, p.bs).astype(np.float64)
    rng = np.random.default_rng(0)
    stream = torch.cuda.Stream()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn, reps):
        with torch.cuda.stream(stream):
            ev0.record(stream)
            for _ in range(reps):
                fn()
            ev1.record(stream)
        ev1.synchronize()
        return ev0.elapsed_time(ev1) / reps

    out = {"commit": args.commit or _commit(), "config": args.config, "smoother": args.smoother, "mat_prec": args.mat_prec, "fuse": word, "nv": nv,
           "n": int(n), "levels": H.n_levels, "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "reps": args.reps,
           "pcg_reps": args.pcg_reps, "note_without_f32": old["note"],
           "float_levels": [l for l in range(H.n_levels) if single.level_extra(l)["gs_f32"]], "k": {}}
    plans = ""
    if d32:
        out["fuse_down_f32"] = word_f
        out["level_plans"] = [dict(single.multi_level_plan(l, word_f), rows=int(single.sizes[l]), gs_down=single.level_paths(l)["gs_down"]) for l in range(H.n_levels - 1)]
        plans = "   levels under " + word_f + ": " + " ".join(
            f"{l}:{q['form']}" + (f"/f32 lanes {q['lanes']} ept {q['ept']} W {q['lw_max_list']} lds {q['lds_bytes']}" if q["form"] != "literal" else
                                  f"({q['note']}" + (f", W {q['lw_max_list']}" if q["lw_max_list"] else "") + ")") for l, q in enumerate(out["level_plans"]))
        # the down stage alone, levels 0 .. 2, k = 2 and 4: the column loop, the float sweep + per-column residual, the NV launch
        out["down_levels"] = {}
        for l in range(min(3, H.n_levels - 1)):
            nl = int(single.sizes[l])
            for k in (2, 4):
                Bl = torch.from_numpy(np.random.default_rng(l).standard_normal((nl, k))).cuda()
                Xl = torch.empty_like(Bl)
                res, tl = {}, {w: [] for w in ("loop", word_e, word_f)}
                for w in tl:
                    res[w] = single.DownMulti(l, Bl, Xl, interleaved=True, fuse=False if w == "loop" else w)[1].clone()
                torch.cuda.synchronize()
                if not (torch.equal(res[word_e], res["loop"]) and torch.equal(res[word_f], res["loop"])):
                    sys.exit(f"bench_multi_rhs: DownMulti of level {l}, k = {k}: the words do not give the column loop's bits")
                for _ in range(args.rounds):
                    for w in tl:
                        tl[w].append(timed(lambda: single.DownMulti(l, Bl, Xl, interleaved=True, fuse=False if w == "loop" else w), args.reps))
                md = {w: statistics.median(v) for w, v in tl.items()}
                out["down_levels"][f"{l}/{k}"] = {w: _stats(v) for w, v in tl.items()}
                print(f"down stage level {l} ({nl} rows, {out['level_plans'][l]['form']}) k = {k}: column loop {md['loop']:.3f} ms  {word_e} {md[word_e]:.3f}  {word_f} {md[word_f]:.3f}"
                      f"  ({word_e})/({word_f}) {md[word_e] / md[word_f]:.2f}", flush=True)
    for k in ks:
        B = rng.standard_normal((k, n)) * pfree
        bs = [torch.from_numpy(np.ascontiguousarray(B[j])).cuda() for j in range(k)]
        xs = [torch.empty_like(b) for b in bs]
        Bi = torch.from_numpy(np.ascontiguousarray(B.T)).cuda()
        X = {key: torch.full_like(Bi, float("nan")) for key in "bcd" + extra}
        calls = {"a": lambda: [single.Mult(bs[j], xs[j]) for j in range(k)],
                 "b": lambda: single.MultMulti(Bi, X["b"], interleaved=True, fuse=word),
                 "c": lambda: single.MultMulti(Bi, X["c"], interleaved=True, fuse=fuse),
                 "d": lambda: double.MultMulti(Bi, X["d"], interleaved=True, fuse=fuse)}
        if d32:
            calls["e"] = lambda: single.MultMulti(Bi, X["e"], interleaved=True, fuse=word_e)
            calls["f"] = lambda: single.MultMulti(Bi, X["f"], interleaved=True, fuse=word_f)
        for fn in calls.values():
            timed(fn, 3)
        torch.cuda.synchronize()
        Xa = torch.stack(xs)
        diff = {key: max(float((X[key][:, j] - Xa[j]).norm() / Xa[j].norm()) for j in range(k)) for key in "bcd" + extra}
        if not (diff["b"] < 1e-12 and diff["c"] == 0.0 and diff["d"] < 1e-5 and all(diff[key] < 1e-12 for key in extra)):
            sys.exit(f"bench_multi_rhs: k = {k}: columns deviate from the single applications: {diff}")
        t = {key: [] for key in calls}
        for _ in range(args.rounds):
            for key, fn in calls.items():
                t[key].append(timed(fn, args.reps))
        med = {key: statistics.median(v) for key, v in t.items()}
        rec = {"max_rel_diff": diff, "cycle": dict({key: _stats(v) for key, v in t.items()}, a_over_b=med["a"] / med["b"], d_over_b=med["d"] / med["b"],
                                                    a_over_c=med["a"] / med["c"], a_spread=(max(t["a"]) - min(t["a"])) / med["a"])}
        line = (f"k = {k}: cycle (a) {med['a']:.3f} ms (spread {rec['cycle']['a_spread']:.3f})  (b) {med['b']:.3f}  (c) {med['c']:.3f}  (d) {med['d']:.3f}  "
                f"(a)/(b) {med['a'] / med['b']:.2f}  (d)/(b) {med['d'] / med['b']:.2f}")
        if d32:
            rec["cycle"].update(a_over_f=med["a"] / med["f"], b_over_f=med["b"] / med["f"], e_over_f=med["e"] / med["f"], d_over_f=med["d"] / med["f"],
                                b_over_f_rounds=[x / y for x, y in zip(t["b"], t["f"])])
            line += (f"  (e) {med['e']:.3f}  (f) {med['f']:.3f}  (a)/(f) {med['a'] / med['f']:.2f}  (b)/(f) {med['b'] / med['f']:.3f}"
                     f" [{min(rec['cycle']['b_over_f_rounds']):.3f} .. {max(rec['cycle']['b_over_f_rounds']):.3f}]  (d)/(f) {med['d'] / med['f']:.2f}")
        if not args.no_pcg:
            cgs, cgd = NativeCGSolver(single, single, tol=1e-8, maxsteps=100), NativeCGSolver(double, double, tol=1e-8, maxsteps=100)
            its = {}

            def pa():
                its["a"] = []
                for j in range(k):
                    xs[j].zero_()
                    cgs.Solve(bs[j], xs[j])
                    its["a"].append(cgs.iterations)

            def multi(key, cg, f):
                def run():
                    X[key].zero_()
                    cg.SolveMulti(Bi, X[key], interleaved=True, fuse=f)
                    its[key] = list(cg.iterations)
                return run

            pcalls = {"a": pa, "b": multi("b", cgs, word), "c": multi("c", cgs, fuse), "d": multi("d", cgd, fuse)}
            if d32:
                pcalls["f"] = multi("f", cgs, word_f)
            with torch.cuda.stream(stream):
                for fn in pcalls.values():
                    fn()
            torch.cuda.synchronize()
            wp = max(float((X["b"][:, j] - xs[j]).norm() / xs[j].norm()) for j in range(k))
            if d32:
                wp = max(wp, max(float((X["f"][:, j] - xs[j]).norm() / xs[j].norm()) for j in range(k)))
            if not wp < 1e-8 or any(abs(x - y) > 1 for x, y in zip(its["a"], its["b"])) or (d32 and its["f"] != its["b"]):
                sys.exit(f"bench_multi_rhs: k = {k}: PCG differs: solutions {wp:.3e}, iterations {its}")
            pt = {key: [] for key in pcalls}
            for _ in range(args.rounds):
                for key, fn in pcalls.items():
                    pt[key].append(timed(fn, args.pcg_reps))
            pm = {key: statistics.median(v) for key, v in pt.items()}
            rec["pcg"] = dict({key: _stats(v) for key, v in pt.items()}, iterations=dict(its), max_rel_diff=wp, a_over_b=pm["a"] / pm["b"],
                              d_over_b=pm["d"] / pm["b"], a_spread=(max(pt["a"]) - min(pt["a"])) / pm["a"])
            line += f"   pcg (a) {pm['a']:.2f} ms (b) {pm['b']:.2f} (d) {pm['d']:.2f}  (a)/(b) {pm['a'] / pm['b']:.2f}  (d)/(b) {pm['d'] / pm['b']:.2f}  iterations {its}"
            if d32:
                rec["pcg"].update(a_over_f=pm["a"] / pm["f"], b_over_f=pm["b"] / pm["f"], d_over_f=pm["d"] / pm["f"])
                line += f"  (f) {pm['f']:.2f}  (a)/(f) {pm['a'] / pm['f']:.2f}  (b)/(f) {pm['b'] / pm['f']:.3f}  (d)/(f) {pm['d'] / pm['f']:.2f}"
        out["k"][str(k)] = rec
        print(line + plans, flush=True)
    path = args.out
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({"out": path, "a_over_b": {k: v["cycle"]["a_over_b"] for k, v in out["k"].items()}}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("nv", nargs="?", type=int, default=None)
    ap.add_argument("--smoother", default="jacobi", choices=["jacobi", "cheby", "gs"])
    ap.add_argument("--degree", type=int, default=2, help="Chebyshev degree")
    ap.add_argument("--config", default="cfg2", choices=["cfg2", "cfg3", "cfg5"])
    ap.add_argument("--k", default="1,2,4,8")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--pcg-reps", type=int, default=30)
    ap.add_argument("--no-pcg", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--down", action="store_true", help="also time the calls with AMGX_MULTI_FUSE_DOWN")
    ap.add_argument("--dia", action="store_true", help="with --down: also time the calls with AMGX_MULTI_FUSE_DOWN_DIA")
    ap.add_argument("--mat-prec", default="double", choices=["double", "single", "single_gs_all", "single_gs"])
    ap.add_argument("--down-f32", action="store_true", help="with --mat-prec single_gs_all: also time the calls with AMGX_MULTI_FUSE_DOWN_F32")
    ap.add_argument("--tag", default="", help="suffix of the result file (runs under environment switches)")
    ap.add_argument("--cycle-only-k", type=int, default=0, help="run nothing but REPS multi-vector cycles of this width (for a kernel trace)")
    args = ap.parse_args()
    if args.dia and not args.down:
        sys.exit("bench_multi_rhs: --dia needs --down")
    if args.down_f32 and not (args.smoother == "gs" and args.config == "cfg2" and args.mat_prec == "single_gs_all"):
        sys.exit("bench_multi_rhs: --down-f32 needs --smoother gs --config cfg2 --mat-prec single_gs_all")
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_multi_rhs: needs a GPU")
    from ngsamg_amd import fem, Matrix
    from ngsamg_amd.hierarchy import Hierarchy
    from ngsamg_amd.device import DeviceAMGMatrix
    from ngsamg_amd.krylov import NativeCGSolver
    nv = args.nv or (215 if args.config == "cfg2" else 126)
    ks = [int(v) for v in args.k.split(",")]
    # handles that are fused only under AMGX_MULTI_FUSE (True) / AMGX_MULTI_FUSE_GS ("gs") / AMGX_MULTI_FUSE_GS_BLOCK ("gs_block")
    if args.smoother == "gs":
        fuse = "gs" if args.config == "cfg2" else "gs_block"
    else:
        fuse = args.smoother != "jacobi" or args.config != "cfg2"
    tag = f"{args.config}_{args.smoother}" + (str(args.degree) if args.smoother == "cheby" else "")
    fuse_down = {False: "down", True: "down", "gs": "gs+down", "gs_block": "gs_block+down"}[fuse]
    fuse_dia = fuse_down + "_dia"
    if args.down:
        tag += ("_f32" if args.mat_prec == "single" else "") + (("_" + args.tag) if args.tag else "")
    if args.out is None:
        if args.mat_prec in ("single_gs_all", "single_gs"):
            args.out = (os.path.join(ROOT, "profiles", "r31", f"multi_down_f32_{args.config}.json") if args.down_f32 else
                        os.path.join(ROOT, "profiles", "r30", f"multi_f32_{args.config}.json"))
        elif args.down:
            args.out = os.path.join(ROOT, "profiles", "r25", f"multi_down_dia_{tag}.json") if args.dia else os.path.join(ROOT, "profiles", "r24", f"multi_down_{tag}.json")
        elif isinstance(fuse, str):
            args.out = os.path.join(ROOT, "profiles", "r21" if fuse == "gs" else "r22", f"multi_gs_{args.config}.json")
        else:
            args.out = os.path.join(ROOT, "profiles", "r14", f"multi_fuse_{tag}.json") if fuse else os.path.join(ROOT, "profiles", "r06", "multi_rhs.json")
    if args.config == "cfg2":
        p = fem.poisson_fast((nv, nv, nv))
        H = Hierarchy(Matrix(p.n, p.n, 1, 1, p.rowptr, p.col, p.val), p.free, p.coords, dim=3, energy=0, max_coarse_size=50)
    else:
        rot = args.config == "cfg5"
        p = fem.elasticity_fast((nv, nv, nv), dirichlet="left", mu=1.0, lam=0.5, rotations=rot)
        H = Hierarchy(Matrix(p.n, p.n, p.bs, p.bs, p.rowptr, p.col, p.val), p.free, p.coords, dim=3, energy=1, max_coarse_size=50,
                      regularize_cmats=0 if rot else 1, spw=1)
    kw = dict(sm_type="cheby", cheb_degree=args.degree) if args.smoother == "cheby" else dict(sm_type="hgs" if args.smoother == "gs" else "jacobi")
    if args.mat_prec in ("single_gs_all", "single_gs"):
        want = "single_gs_all" if args.config == "cfg2" else "single_gs"
        if args.smoother != "gs" or args.mat_prec != want:
            sys.exit(f"bench_multi_rhs: --mat-prec {args.mat_prec} needs --smoother gs and --config " + ("cfg2" if args.mat_prec == "single_gs_all" else "cfg3 | cfg5"))
        return _f32(args, H, p, kw, fuse, ks, nv)
    if args.mat_prec != "double":
        kw["mat_prec"] = args.mat_prec
    free0, _ = torch.cuda.mem_get_info()
    dev = DeviceAMGMatrix(H, device=0, **kw)
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info()
    n = p.n * p.bs
    pfree = np.repeat(p.free, p.bs).astype(np.float64)
    rng = np.random.default_rng(0)
    stream = torch.cuda.Stream()                               # (the legacy default stream cannot be captured into a graph)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn, reps):
        with torch.cuda.stream(stream):
            ev0.record(stream)
            for _ in range(reps):
                fn()
            ev1.record(stream)
        ev1.synchronize()
        return ev0.elapsed_time(ev1) / reps

    if args.cycle_only_k:
        k = args.cycle_only_k
        Bi = torch.from_numpy(rng.standard_normal((n, k)) * pfree[:, None]).cuda()
        Xi = torch.empty_like(Bi)
        torch.cuda.synchronize()
        print("ms per multi cycle:", timed(lambda: dev.MultMulti(Bi, Xi, interleaved=True, fuse=fuse), args.reps))
        if args.down:
            print("ms per multi cycle with AMGX_MULTI_FUSE_DOWN:", timed(lambda: dev.MultMulti(Bi, Xi, interleaved=True, fuse=fuse_down), args.reps))
        if args.dia:
            print("ms per multi cycle with AMGX_MULTI_FUSE_DOWN_DIA:", timed(lambda: dev.MultMulti(Bi, Xi, interleaved=True, fuse=fuse_dia), args.reps))
        return

    if isinstance(fuse, str) and dev.multi_plan(4, fuse=fuse)["fused"] != 1:
        flag = "AMGX_MULTI_FUSE_GS" if fuse == "gs" else "AMGX_MULTI_FUSE_GS_BLOCK"
        sys.exit(f"bench_multi_rhs: the handle is not fused under {flag}: " + dev.multi_plan(4, fuse=fuse)["note"])
    out = {"commit": args.commit or _commit(), "config": args.config, "smoother": args.smoother, "degree": args.degree if args.smoother == "cheby" else 0,
           "fuse": fuse, "nv": nv, "n": int(n), "levels": H.n_levels, "cycle_info": dev.cycle_info(),
           "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "reps": args.reps, "pcg_reps": args.pcg_reps,
           "handle_bytes": int(free0 - free1), "k": {}}
    if isinstance(fuse, str):                                  # the forms under test and the matrix bytes of the byte model, per smoothed level
        keys = ("gs_form", "gs_lanes", "gs_threads", "gs_block", "gs_colors", "gs_block_colors", "gs_split", "gs_narrow", "gs_mid", "gs_lw", "gs_down")
        out["levels_gs"] = [dict({key: dev.level_paths(l)[key] for key in keys}, rows=int(dev.sizes[l]),
                                 A_stream_bytes=dev.matrix_info(l, "A")["stream_bytes"]) for l in range(H.n_levels - 1)]
    plans = ""

    def level_plans(word):
        return [dict(dev.multi_level_plan(l, word), rows=int(dev.sizes[l]), kernel=dev.level_paths(l)["kernel"], compact=dev.level_paths(l)["compact"],
                     gs_down=dev.level_paths(l)["gs_down"]) for l in range(H.n_levels - 1)]

    def plan_text(lp):
        return " ".join(f"{l}:{q['form']}" + (f"/{q['mode']}" + ("+Q" if q["folded_up"] else "") + ("/f32" if q["float_image"] else "")
                                              if q["form"] != "literal" else f"({q['note']})") for l, q in enumerate(lp))

    if args.down:
        out["fuse_down"] = fuse_down
        out["level_plans"] = level_plans(fuse_down)
        plans = "   levels: " + plan_text(out["level_plans"])
    if args.dia:
        out["fuse_dia"] = fuse_dia
        out["level_plans_dia"] = level_plans(fuse_dia)
        plans += "   levels with " + fuse_dia + ": " + plan_text(out["level_plans_dia"])
    for k in ks:
        info = dev.multi_plan(k, fuse=fuse)
        B = rng.standard_normal((k, n)) * pfree
        bs = [torch.from_numpy(np.ascontiguousarray(B[j])).cuda() for j in range(k)]
        xs = [torch.empty_like(b) for b in bs]
        Bi = torch.from_numpy(np.ascontiguousarray(B.T)).cuda()
        Xi = torch.full_like(Bi, float("nan"))
        Bc = torch.from_numpy(B).cuda()
        Xc = torch.full_like(Bc, float("nan"))
        torch.cuda.synchronize()

        def a():
            for j in range(k):
                dev.Mult(bs[j], xs[j])

        def b():
            dev.MultMulti(Bi, Xi, interleaved=True, fuse=fuse)

        def c():
            dev.MultMulti(Bc, Xc, fuse=fuse)

        Xd = torch.full_like(Bi, float("nan"))

        def d():
            dev.MultMulti(Bi, Xd, interleaved=True, fuse=fuse_down)

        Xe = torch.full_like(Bi, float("nan"))

        def e():
            dev.MultMulti(Bi, Xe, interleaved=True, fuse=fuse_dia)

        m0, _ = torch.cuda.mem_get_info()
        for fn in (a, b, c) + ((d,) if args.down else ()) + ((e,) if args.dia else ()):      # warm-up: captures the graphs, allocates the work space
            timed(fn, 3)
        torch.cuda.synchronize()
        m1, _ = torch.cuda.mem_get_info()
        # (b) equals (a) column by column before any time counts
        Xa = torch.stack(xs)
        worst = 0.0
        for j in range(k):
            for got in (Xi[:, j], Xc[j]) + ((Xd[:, j],) if args.down else ()) + ((Xe[:, j],) if args.dia else ()):
                worst = max(worst, float((got - Xa[j]).norm() / Xa[j].norm()))
        if not worst < 1e-12:
            sys.exit(f"bench_multi_rhs: k = {k}: multi-vector cycle deviates from the single-vector one by {worst:.3e}")
        ta, tb, tc, td, te = [], [], [], [], []
        for _ in range(args.rounds):                            # alternating blocks
            ta.append(timed(a, args.reps))
            tb.append(timed(b, args.reps))
            tc.append(timed(c, args.reps))
            if args.down:
                td.append(timed(d, args.reps))
            if args.dia:
                te.append(timed(e, args.reps))
        rec = {"multi_info": info, "work_bytes_allocated": int(m0 - m1), "max_rel_diff": worst,
               "cycle": {"single_x_k": _stats(ta), "multi_interleaved": _stats(tb), "multi_colmajor": _stats(tc),
                         "ratio_rounds": [x / y for x, y in zip(ta, tb)], "ratio_median": statistics.median(ta) / statistics.median(tb),
                         "ratio_colmajor_median": statistics.median(ta) / statistics.median(tc),
                         "multi_wins_every_round": all(x > y for x, y in zip(ta, tb))}}
        if args.down:                                           # (the yardstick of (d) is (b) of the same round)
            rec["multi_level_plan_bytes"] = dev.multi_plan(k, fuse=fuse_down)["work_bytes"]
            rec["cycle"].update({"multi_down": _stats(td), "ratio_down_median": statistics.median(ta) / statistics.median(td),
                                 "multi_over_down_rounds": [x / y for x, y in zip(tb, td)],
                                 "multi_over_down_median": statistics.median(tb) / statistics.median(td)})
        if args.dia:                                            # (the yardstick of (e) is (b) of the same round, too)
            rec["multi_level_plan_bytes_dia"] = dev.multi_plan(k, fuse=fuse_dia)["work_bytes"]
            rec["cycle"].update({"multi_dia": _stats(te), "ratio_dia_median": statistics.median(ta) / statistics.median(te),
                                 "multi_over_dia_rounds": [x / y for x, y in zip(tb, te)],
                                 "multi_over_dia_median": statistics.median(tb) / statistics.median(te),
                                 "multi_spread": (max(tb) - min(tb)) / statistics.median(tb)})
        if not args.no_pcg:
            cg = NativeCGSolver(dev, dev, tol=1e-8, maxsteps=100)
            its_a = []

            def pa():
                its_a.clear()
                for j in range(k):
                    xs[j].zero_()
                    cg.Solve(bs[j], xs[j])
                    its_a.append(cg.iterations)

            def pb():
                Xi.zero_()
                cg.SolveMulti(Bi, Xi, interleaved=True, fuse=fuse)

            with torch.cuda.stream(stream):
                pa()
                pb()
            torch.cuda.synchronize()
            its_b = list(cg.iterations)

            def pd():
                Xd.zero_()
                cg.SolveMulti(Bi, Xd, interleaved=True, fuse=fuse_down)

            if args.down:
                with torch.cuda.stream(stream):
                    pd()
                torch.cuda.synchronize()
                its_d = list(cg.iterations)
                wd = max(float((Xd[:, j] - xs[j]).norm() / xs[j].norm()) for j in range(k))
                if not wd < 1e-8 or any(abs(x - y) > 1 for x, y in zip(its_b, its_d)):
                    sys.exit(f"bench_multi_rhs: k = {k}: PCG with AMGX_MULTI_FUSE_DOWN differs: solutions {wd:.3e}, iterations {its_b} vs {its_d}")
            def pe():
                Xe.zero_()
                cg.SolveMulti(Bi, Xe, interleaved=True, fuse=fuse_dia)

            if args.dia:
                with torch.cuda.stream(stream):
                    pe()
                torch.cuda.synchronize()
                its_e = list(cg.iterations)
                we = max(float((Xe[:, j] - xs[j]).norm() / xs[j].norm()) for j in range(k))
                if not we < 1e-8 or any(abs(x - y) > 1 for x, y in zip(its_b, its_e)):
                    sys.exit(f"bench_multi_rhs: k = {k}: PCG with AMGX_MULTI_FUSE_DOWN_DIA differs: solutions {we:.3e}, iterations {its_b} vs {its_e}")
            wp = max(float((Xi[:, j] - xs[j]).norm() / xs[j].norm()) for j in range(k))
            if not wp < 1e-8 or any(abs(x - y) > 1 for x, y in zip(its_a, its_b)):
                sys.exit(f"bench_multi_rhs: k = {k}: PCG differs: solutions {wp:.3e}, iterations {its_a} vs {its_b}")
            pta, ptb, ptd, pte = [], [], [], []
            for _ in range(args.rounds):
                pta.append(timed(pa, args.pcg_reps))
                ptb.append(timed(pb, args.pcg_reps))
                if args.down:
                    ptd.append(timed(pd, args.pcg_reps))
                if args.dia:
                    pte.append(timed(pe, args.pcg_reps))
            rec["pcg"] = {"iterations_single": list(its_a), "iterations_multi": its_b, "max_rel_diff": wp, "single_x_k": _stats(pta),
                          "multi_interleaved": _stats(ptb), "ratio_rounds": [x / y for x, y in zip(pta, ptb)],
                          "ratio_median": statistics.median(pta) / statistics.median(ptb),
                          "multi_wins_every_round": all(x > y for x, y in zip(pta, ptb))}
            if args.down:
                rec["pcg"].update({"iterations_down": its_d, "multi_down": _stats(ptd), "ratio_down_median": statistics.median(pta) / statistics.median(ptd),
                                   "multi_over_down_rounds": [x / y for x, y in zip(ptb, ptd)],
                                   "multi_over_down_median": statistics.median(ptb) / statistics.median(ptd)})
            if args.dia:
                rec["pcg"].update({"iterations_dia": its_e, "multi_dia": _stats(pte), "ratio_dia_median": statistics.median(pta) / statistics.median(pte),
                                   "multi_over_dia_rounds": [x / y for x, y in zip(ptb, pte)],
                                   "multi_over_dia_median": statistics.median(ptb) / statistics.median(pte),
                                   "multi_spread": (max(ptb) - min(ptb)) / statistics.median(ptb)})
        out["k"][str(k)] = rec
        print(f"k = {k}: cycle (a) {statistics.median(ta):.3f} ms  (b) {statistics.median(tb):.3f} ms  (b') {statistics.median(tc):.3f} ms  "
              f"ratio (a)/(b) {rec['cycle']['ratio_median']:.2f}" + (f"   pcg ratio {rec['pcg']['ratio_median']:.2f}" if "pcg" in rec else "") +
              (f"   (d) {statistics.median(td):.3f} ms  (a)/(d) {rec['cycle']['ratio_down_median']:.2f}  (b)/(d) {rec['cycle']['multi_over_down_median']:.3f}"
               f" [{min(rec['cycle']['multi_over_down_rounds']):.3f} .. {max(rec['cycle']['multi_over_down_rounds']):.3f}]" +
               (f"   pcg (b)/(d) {rec['pcg']['multi_over_down_median']:.3f}" if "pcg" in rec else "") if args.down else "") +
              (f"   (e) {statistics.median(te):.3f} ms  (a)/(e) {rec['cycle']['ratio_dia_median']:.2f}  (b)/(e) {rec['cycle']['multi_over_dia_median']:.3f}"
               f" [{min(rec['cycle']['multi_over_dia_rounds']):.3f} .. {max(rec['cycle']['multi_over_dia_rounds']):.3f}]  (b) spread {rec['cycle']['multi_spread']:.3f}" +
               (f"   pcg (a)/(e) {rec['pcg']['ratio_dia_median']:.2f}  (b)/(e) {rec['pcg']['multi_over_dia_median']:.3f}  (b) spread {rec['pcg']['multi_spread']:.3f}"
                if "pcg" in rec else "") + f"   work space {rec['multi_level_plan_bytes_dia'] / 2**20:.0f} MiB" if args.dia else "") + plans, flush=True)
        del bs, xs, Bi, Xi, Bc, Xc, Xd, Xe
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({"out": args.out, "ratios": {k: v["cycle"]["ratio_median"] for k, v in out["k"].items()}}))


if __name__ == "__main__":
    main()
