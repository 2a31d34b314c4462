#!/usr/bin/env python3
"""Single-precision matrix storage of the Chebyshev levels (mat_prec = "single") against double: one process, one
hierarchy, alternating rounds.

    python tools/bench_mat_prec.py [nv] [--config cfg2|cfg3|cfg5] [--rounds 5] [--reps 20] [--out FILE] [--commit ID]

Builds the hierarchy of the benchmark configuration as bench.py does (cfg2: fem.poisson_fast((nv,)*3, jitter 0.2), nv = 215; cfg3 /
cfg5: fem.elasticity_fast((nv,)*3) without / with rotations, nv = 126; SPW hierarchy, max_coarse_size 50) and, for Chebyshev degree 1
and 2, one double and one single handle on it with the same interval (the double handle's estimate).  Per handle and round:
applications per second (device vectors, graph replay, one stream), the rounds of the two handles alternating; once per handle:
amgx_pcg iterations and time to 1e-8; per level: amgx_time_op 10 (the fused Chebyshev step) and 5 (pre-smoothing + restriction) for
both handles, alternating, the stream bytes of "A" and "A32", and the device memory each handle took.  Cross-run numbers differ by
several per cent between machines and processes, so only the lines of one run compare.  Needs a GPU."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _commit():
    try:
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        return "unknown"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("nv", nargs="?", type=int, default=None)
    ap.add_argument("--config", default="cfg2", choices=["cfg2", "cfg3", "cfg5"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--op-reps", type=int, default=20)
    ap.add_argument("--pcg-reps", type=int, default=3)
    ap.add_argument("--degrees", default="1,2")
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--step-only", type=int, default=0, help="run nothing but this many op-10 launches per handle on level 0 (for a kernel trace)")
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_mat_prec: needs a GPU")
    from ngsamg_amd import fem, Matrix
    from ngsamg_amd.hierarchy import Hierarchy
    from ngsamg_amd.device import DeviceAMGMatrix
    from ngsamg_amd.krylov import NativeCGSolver
    nv = args.nv or (215 if args.config == "cfg2" else 126)
    out_path = args.out or os.path.join(ROOT, "profiles", "r08", f"mat_prec_{args.config}.json")
    t0 = time.time()
    if args.config == "cfg2":
        p = fem.poisson_fast((nv, nv, nv), dirichlet="right|top", jitter=0.2, seed=1)
        H = Hierarchy(Matrix(p.n, p.n, 1, 1, p.rowptr, p.col, p.val), p.free, p.coords, dim=3, energy=0, max_coarse_size=50, max_levels=10, spw=1)
    else:
        rot = args.config == "cfg5"
        p = fem.elasticity_fast((nv, nv, nv), dirichlet="left", mu=1.0, lam=0.5, rotations=rot)
        H = Hierarchy(Matrix(p.n, p.n, p.bs, p.bs, p.rowptr, p.col, p.val), p.free, p.coords, dim=3, energy=1, max_coarse_size=50,
                      regularize_cmats=0 if rot else 1, spw=1)
    print(f"hierarchy: {[lv.n for lv in H.levels]} block sizes {[lv.bs for lv in H.levels]} ({time.time() - t0:.1f} s)", flush=True)
    n = p.n * p.bs
    free = np.repeat(p.free, p.bs).astype(np.float64)
    rng = np.random.default_rng(0)
    b = torch.from_numpy(rng.standard_normal(n) * free).cuda()
    load = torch.from_numpy(np.ascontiguousarray(np.asarray(p.load, dtype=np.float64).reshape(-1))).cuda()
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

    def create(**kw):
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        t1 = time.time()
        dev = DeviceAMGMatrix(H, device=0, sm_type="cheby", **kw)
        torch.cuda.synchronize()
        return dev, int(free0 - torch.cuda.mem_get_info()[0]), time.time() - t1

    degrees = [int(v) for v in args.degrees.split(",")]
    if args.step_only:
        dbl, _, _ = create(cheb_degree=2)
        lm = [dbl.smoother_info(l)["lambda_max"] for l in range(H.n_levels - 1)] + [1.0]
        sgl, _, _ = create(cheb_degree=2, cheb_lambda_max=lm, mat_prec="single")
        print("op 10 (ms): double", dbl.time_op(0, 10, args.step_only), " single", sgl.time_op(0, 10, args.step_only))
        print("op 5 (ms): double", dbl.time_op(0, 5, args.step_only), " single", sgl.time_op(0, 5, args.step_only))
        return

    out = {"commit": args.commit or _commit(), "config": args.config, "nv": nv, "n": int(n), "levels": [int(lv.n) for lv in H.levels],
           "block_sizes": [int(lv.bs) for lv in H.levels], "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "reps": args.reps,
           "degrees": {}}
    summary = {}
    for degree in degrees:
        dbl, mem_d, t_d = create(cheb_degree=degree)
        lm = [dbl.smoother_info(l)["lambda_max"] for l in range(H.n_levels - 1)] + [1.0]
        sgl, mem_s, t_s = create(cheb_degree=degree, cheb_lambda_max=lm, mat_prec="single")
        handles = {"double": dbl, "single": sgl}
        print(f"degree {degree}: handles created in {t_d:.1f} / {t_s:.1f} s, device memory {mem_d / 1e9:.2f} / {mem_s / 1e9:.2f} GB", flush=True)
        xs = {k: torch.empty_like(b) for k in handles}
        for k, dev in handles.items():                            # warm-up: captures the graphs
            timed(lambda: dev.Mult(b, xs[k]), 3)
        torch.cuda.synchronize()
        times = {k: [] for k in handles}
        for _ in range(args.rounds):                               # alternating rounds
            for k, dev in handles.items():
                times[k].append(timed(lambda: dev.Mult(b, xs[k]), args.reps))
        rec = {"device_memory_bytes": {"double": mem_d, "single": mem_s}, "lambda_max": lm[:-1], "handles": {}}
        for k, dev in handles.items():
            h = {"cycle_ms": {"median": statistics.median(times[k]), "min": min(times[k]), "max": max(times[k]), "rounds": times[k]},
                 "applications_per_s": 1000.0 / statistics.median(times[k]), "applications_per_s_rounds": [1000.0 / t for t in times[k]],
                 "cycle_info": dev.cycle_info()}
            cg = NativeCGSolver(dev, dev, tol=1e-8, maxsteps=300)
            x = torch.zeros_like(load)
            pt = []
            with torch.cuda.stream(stream):
                cg.Solve(load, x)                                  # warm-up (graph of the solver's vectors)
            torch.cuda.synchronize()
            for _ in range(args.pcg_reps):
                x.zero_()
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                with torch.cuda.stream(stream):
                    cg.Solve(load, x)
                torch.cuda.synchronize()
                pt.append((time.perf_counter() - t1) * 1e3)
            conv = bool(cg.errors[-1] <= 1e-8 * cg.errors[0])
            h["pcg"] = {"iterations": int(cg.iterations), "converged": conv, "ms_median": statistics.median(pt), "ms_min": min(pt),
                        "final_rel_err": float(cg.errors[-1] / cg.errors[0])}
            rec["handles"][k] = h
        rec["single_not_slower_in_every_round"] = all(s <= d for s, d in zip(times["single"], times["double"]))
        lv = []
        for l in range(H.n_levels - 1):
            a, a32 = dbl.matrix_info(l, "A"), sgl.matrix_info(l, "A32")
            e = {"level": l, "n": int(H.levels[l].n), "bs": int(H.levels[l].bs), "A": a, "A32": a32, "paths_kernel": sgl.level_paths(l)["kernel"]}
            for op, key in ((10, "op10_cheby_step_ms"), (5, "op5_down_ms")):
                t = {"double": [], "single": []}
                for _ in range(args.rounds):                       # alternating
                    for k, dev in handles.items():
                        t[k].append(dev.time_op(l, op, args.op_reps))
                e[key] = {k: statistics.median(v) for k, v in t.items()}
                e[key]["single_over_double"] = e[key]["single"] / e[key]["double"]
                if a32["fmt"] is not None and op == 10:
                    e["op10_GBps"] = {"double": a["stream_bytes"] / e[key]["double"] / 1e6, "single": a32["stream_bytes"] / e[key]["single"] / 1e6}
            lv.append(e)
            print(f"  level {l}: n {e['n']} bs {e['bs']} A {a['fmt']}/{a['lanes']} A32 {a32['fmt']}  bytes {a['stream_bytes']} -> {a32['stream_bytes']}  "
                  f"op10 {e['op10_cheby_step_ms']['double']:.4f} -> {e['op10_cheby_step_ms']['single']:.4f} ms  "
                  f"op5 {e['op5_down_ms']['double']:.4f} -> {e['op5_down_ms']['single']:.4f} ms", flush=True)
        rec["per_level"] = lv
        out["degrees"][str(degree)] = rec
        hd, hs = rec["handles"]["double"], rec["handles"]["single"]
        print(f"degree {degree}: {hd['applications_per_s']:.1f} -> {hs['applications_per_s']:.1f} applications/s, PCG {hd['pcg']['iterations']} / "
              f"{hs['pcg']['iterations']} iterations in {hd['pcg']['ms_median']:.1f} / {hs['pcg']['ms_median']:.1f} ms, single not slower in every round: "
              f"{rec['single_not_slower_in_every_round']}", flush=True)
        summary[str(degree)] = {"applications_per_s": [round(hd["applications_per_s"], 1), round(hs["applications_per_s"], 1)],
                                "pcg_iterations": [hd["pcg"]["iterations"], hs["pcg"]["iterations"]],
                                "pcg_ms": [round(hd["pcg"]["ms_median"], 1), round(hs["pcg"]["ms_median"], 1)],
                                "device_memory_GB": [round(mem_d / 1e9, 2), round(mem_s / 1e9, 2)]}
        del dbl, sgl, handles
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({"out": out_path, "double_single": summary}))


if __name__ == "__main__":
    main()
