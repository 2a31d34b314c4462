#!/usr/bin/env python3
"""Chebyshev smoother against Jacobi and Gauss-Seidel: one process, one hierarchy, alternating rounds.

    python tools/bench_cheby.py [nv] [--config cfg2|cfg3|cfg5] [--rounds 5] [--reps 20] [--out FILE] [--commit ID]

Builds the hierarchy of the benchmark configuration as bench.py does (cfg2: fem.poisson_fast((nv,)*3, jitter 0.2), nv = 215; cfg3 /
cfg5: fem.elasticity_fast((nv,)*3) without / with rotations, nv = 126; SPW hierarchy, max_coarse_size 50) and creates five handles on
it: Jacobi (omega 0.9), Gauss-Seidel in its default form ("hgs": block-hybrid / block-coloured), Chebyshev of degree 1, 2 and 3 with
the interval estimated on the device.  Per handle and round: applications per second (device vectors, graph replay, one stream);
once per handle: amgx_pcg iterations and time to 1e-8; per level: amgx_time_op 10 (the fused Chebyshev step) next to op 1 (the
fused Jacobi step) and op 0 (the residual).  Cross-run numbers differ by several per cent between machines and processes
(DESIGN.md 6), so only the lines of one run compare.  Needs a GPU."""
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
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--step-only", type=int, default=0, help="run nothing but this many op-10 and op-1 launches on level 0 (for a kernel trace)")
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_cheby: needs a GPU")
    from ngsamg_amd import fem, Matrix
    from ngsamg_amd.hierarchy import Hierarchy
    from ngsamg_amd.device import DeviceAMGMatrix
    from ngsamg_amd.krylov import NativeCGSolver
    nv = args.nv or (215 if args.config == "cfg2" else 126)
    out_path = args.out or os.path.join(ROOT, "profiles", "r07", f"cheby_{args.config}.json")
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

    if args.step_only:
        dev = DeviceAMGMatrix(H, sm_type="cheby", device=0)
        jac = DeviceAMGMatrix(H, sm_type="jacobi", device=0)
        print("op 10 (ms):", dev.time_op(0, 10, args.step_only), " op 1 (ms):", jac.time_op(0, 1, args.step_only))
        return

    specs = [("jacobi", dict(sm_type="jacobi")), ("gs", dict(sm_type="hgs")), ("cheby1", dict(sm_type="cheby", cheb_degree=1)),
             ("cheby2", dict(sm_type="cheby", cheb_degree=2)), ("cheby3", dict(sm_type="cheby", cheb_degree=3))]
    handles = {}
    for name, kw in specs:
        t1 = time.time()
        handles[name] = DeviceAMGMatrix(H, device=0, **kw)
        torch.cuda.synchronize()
        print(f"handle {name}: {time.time() - t1:.1f} s", flush=True)
    xs = {name: torch.empty_like(b) for name in handles}
    out = {"commit": args.commit or _commit(), "config": args.config, "nv": nv, "n": int(n), "levels": [int(lv.n) for lv in H.levels],
           "block_sizes": [int(lv.bs) for lv in H.levels], "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "reps": args.reps,
           "handles": {}}
    for name, dev in handles.items():                          # warm-up: captures the graphs
        timed(lambda: dev.Mult(b, xs[name]), 3)
    torch.cuda.synchronize()
    times = {name: [] for name in handles}
    for _ in range(args.rounds):                                # alternating rounds
        for name, dev in handles.items():
            times[name].append(timed(lambda: dev.Mult(b, xs[name]), args.reps))
    for name, dev in handles.items():
        rec = {"cycle_ms": {"median": statistics.median(times[name]), "min": min(times[name]), "max": max(times[name]), "rounds": times[name]},
               "applications_per_s": 1000.0 / statistics.median(times[name]), "cycle_info": dev.cycle_info()}
        cg = NativeCGSolver(dev, dev, tol=1e-8, maxsteps=300)
        x = torch.zeros_like(load)
        pt = []
        with torch.cuda.stream(stream):
            cg.Solve(load, x)                                   # warm-up (graph of the solver's vectors)
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
        rec["pcg"] = {"iterations": int(cg.iterations), "converged": conv, "ms_median": statistics.median(pt), "ms_min": min(pt),
                      "final_rel_err": float(cg.errors[-1] / cg.errors[0])}
        lv = []
        for l in range(H.n_levels - 1):
            e = {"level": l, "smoother": dev.smoother_info(l), "paths_kernel": dev.level_paths(l)["kernel"], "op0_residual_ms": dev.time_op(l, 0, args.op_reps)}
            if name == "jacobi":
                e["op1_jacobi_step_ms"] = dev.time_op(l, 1, args.op_reps)
            if name.startswith("cheby"):
                e["op10_cheby_step_ms"] = dev.time_op(l, 10, args.op_reps)
            e["op5_down_ms"] = dev.time_op(l, 5, args.op_reps)
            e["op6_up_ms"] = dev.time_op(l, 6, args.op_reps)
            lv.append(e)
        rec["per_level"] = lv
        out["handles"][name] = rec
        print(f"{name}: {rec['applications_per_s']:.1f} applications/s, cycle {rec['cycle_ms']['median']:.3f} ms, PCG {rec['pcg']['iterations']} iterations"
              f"{'' if conv else ' (NOT converged)'} in {rec['pcg']['ms_median']:.1f} ms", flush=True)
    # the fused Chebyshev step next to the fused Jacobi step, same process, alternating
    ratios = []
    for l in range(H.n_levels - 1):
        a, c = [], []
        for _ in range(args.rounds):
            a.append(handles["jacobi"].time_op(l, 1, args.op_reps))
            c.append(handles["cheby2"].time_op(l, 10, args.op_reps))
        ratios.append({"level": l, "op1_ms": statistics.median(a), "op10_ms": statistics.median(c), "ratio": statistics.median(c) / statistics.median(a)})
    out["op10_over_op1"] = ratios
    print("op 10 / op 1 per level:", [round(r["ratio"], 3) for r in ratios], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({"out": out_path, "applications_per_s": {k: round(v["applications_per_s"], 1) for k, v in out["handles"].items()},
                      "pcg_iterations": {k: v["pcg"]["iterations"] for k, v in out["handles"].items()},
                      "pcg_ms": {k: round(v["pcg"]["ms_median"], 1) for k, v in out["handles"].items()}}))


if __name__ == "__main__":
    main()
