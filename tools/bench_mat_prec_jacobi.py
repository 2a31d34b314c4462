#!/usr/bin/env python3
"""Single-precision images of the scalar Jacobi levels (jacobi_prec = "single") against double: one process, one
hierarchy, alternating rounds.

    python tools/bench_mat_prec_jacobi.py [nv] --config cfg2 [--rounds 5] [--reps 20] [--out FILE] [--commit ID]

Builds the hierarchy of the benchmark configuration as bench.py does (cfg2: fem.poisson_fast((nv,)*3, jitter 0.2, seed 1), nv = 215;
SPW hierarchy, max_coarse_size 50, Jacobi V(1,1)) and one double and one single handle on it.  Per handle and round: applications
per second (device vectors, graph replay, one stream), the rounds of the two handles alternating; once per handle: amgx_pcg
iterations and time to 1e-8; per level, alternating: amgx_time_op 5 (the down pass), 6 (the way up) and 8 (the fused down kernel inside
the cycle), jacobi_prec_info, and the device memory each handle took.  Reports the medians and the spread of the double handle over
the rounds beside the byte-model figure (the level-0 down kernel streams 0.556 GB of upper diagonals out of the 1.95 GB
it moves at 215^3; float values take 0.28 GB of that away).  Cross-run numbers differ by several per cent between machines and
processes, so only the lines of one run compare.  Needs a GPU."""
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
    ap.add_argument("nv", nargs="?", type=int, default=215)
    ap.add_argument("--config", default="cfg2", choices=["cfg2"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--op-reps", type=int, default=10)
    ap.add_argument("--pcg-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_mat_prec_jacobi: needs a GPU")
    from ngsamg_amd import fem, Matrix
    from ngsamg_amd.hierarchy import Hierarchy
    from ngsamg_amd.device import DeviceAMGMatrix
    from ngsamg_amd.krylov import NativeCGSolver
    from ngsamg_amd._lib import NgsAMGError
    nv = args.nv
    knobs = {k: v for k, v in os.environ.items() if k.startswith("AMGX_")}
    out_path = args.out or os.path.join(ROOT, "profiles", "r26", f"mat_prec_jacobi_{args.config}.json")
    t0 = time.time()
    p = fem.poisson_fast((nv, nv, nv), dirichlet="right|top", jitter=0.2, seed=1)
    H = Hierarchy(Matrix(p.n, p.n, 1, 1, p.rowptr, p.col, p.val), p.free, p.coords, dim=3, energy=0, max_coarse_size=50, max_levels=10, spw=1)
    print(f"hierarchy: {[lv.n for lv in H.levels]} block sizes {[lv.bs for lv in H.levels]} ({time.time() - t0:.1f} s)", flush=True)
    n = p.n * p.bs
    free = np.repeat(p.free, p.bs).astype(np.float64)
    rng = np.random.default_rng(0)
    b = torch.from_numpy(rng.standard_normal(n) * free).cuda()
    load = b
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
        dev = DeviceAMGMatrix(H, device=0, sm_type="jacobi", **kw)
        torch.cuda.synchronize()
        return dev, int(free0 - torch.cuda.mem_get_info()[0]), time.time() - t1

    dbl, mem_d, t_d = create()
    sgl, mem_s, t_s = create(jacobi_prec="single")
    handles = {"double": dbl, "single": sgl}
    print(f"handles created in {t_d:.1f} / {t_s:.1f} s, device memory {mem_d / 1e9:.2f} / {mem_s / 1e9:.2f} GB", flush=True)
    out = {"commit": args.commit or _commit(), "config": args.config, "smoother": "jacobi", "environment": knobs, "nv": nv, "n": int(n),
           "levels": [int(lv.n) for lv in H.levels], "block_sizes": [int(lv.bs) for lv in H.levels], "device": torch.cuda.get_device_name(0),
           "rounds": args.rounds, "reps": args.reps,
           "byte_model": {"level0_down_kernel_GB_measured_fp64": 1.95, "of_which_upper_diagonals_GB": 0.556, "float_values_save_GB": 0.278,
                          "note": "model values at 215^3 (DESIGN.md 5.1b, 5.20), not measurements of this run"},
           "device_memory_bytes": {"double": mem_d, "single": mem_s}, "handles": {}}
    xs = {k: torch.empty_like(b) for k in handles}
    for k, dev in handles.items():                            # warm-up: captures the graphs
        timed(lambda: dev.Mult(b, xs[k]), 3)
    torch.cuda.synchronize()
    times = {k: [] for k in handles}
    for _ in range(args.rounds):                               # alternating rounds
        for k, dev in handles.items():
            times[k].append(timed(lambda: dev.Mult(b, xs[k]), args.reps))
    change = float(torch.linalg.norm(xs["single"] - xs["double"]) / torch.linalg.norm(xs["double"]))
    for k, dev in handles.items():
        h = {"cycle_ms": {"median": statistics.median(times[k]), "min": min(times[k]), "max": max(times[k]), "rounds": times[k],
                          "spread_rel": (max(times[k]) - min(times[k])) / statistics.median(times[k])},
             "applications_per_s": 1000.0 / statistics.median(times[k]), "cycle_info": dev.cycle_info()}
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
        h["pcg"] = {"iterations": int(cg.iterations), "converged": bool(cg.errors[-1] <= 1e-8 * cg.errors[0]), "ms_median": statistics.median(pt),
                    "ms_min": min(pt), "final_rel_err": float(cg.errors[-1] / cg.errors[0])}
        out["handles"][k] = h
    out["relative_change_of_one_application"] = change
    out["single_not_slower_in_every_round"] = all(s <= d for s, d in zip(times["single"], times["double"]))
    lv = []
    with torch.cuda.stream(stream):                            # (op 11 needs a stream that is not the default one)
        for l in range(H.n_levels - 1):
            lp, ji = sgl.level_paths(l), sgl.jacobi_prec_info(l)
            e = {"level": l, "n": int(H.levels[l].n), "kernel": lp["kernel"], "compact": lp["compact"], "folded": lp["folded"],
                 "jacobi_prec_info": {k: (list(v) if isinstance(v, tuple) else v) for k, v in ji.items()},
                 "A": dbl.matrix_info(l, "A"), "Apre": dbl.matrix_info(l, "Apre"), "Q": dbl.matrix_info(l, "Q"), "QLW": dbl.matrix_info(l, "QLW")}
            for op, key in ((5, "op5_down_ms"), (6, "op6_up_ms"), (8, "op8_down_kernel_in_cycle_ms")):
                t = {"double": [], "single": []}
                try:
                    for _ in range(args.rounds):               # alternating
                        for k, dev in handles.items():
                            t[k].append(dev.time_op(l, op, args.op_reps))
                except NgsAMGError as err:                     # (a level without a fused down kernel)
                    e[key] = {"unmeasured": str(err)}
                    continue
                e[key] = {k: statistics.median(v) for k, v in t.items()}
                e[key]["single_over_double"] = e[key]["single"] / e[key]["double"]
            lv.append(e)

            def fmt(key):
                v = e[key]
                return "-" if "unmeasured" in v else f"{v['double']:.4f} -> {v['single']:.4f} ms ({v['single_over_double']:.2f})"
            print(f"  level {l}: n {e['n']} {e['kernel']} f32 {ji['f32']} images {','.join(ji['images'])} ({ji['bytes']} B, released {ji['released']} B)  "
                  f"op5 {fmt('op5_down_ms')}  op6 {fmt('op6_up_ms')}  op8 {fmt('op8_down_kernel_in_cycle_ms')}", flush=True)
    out["per_level"] = lv
    hd, hs = out["handles"]["double"], out["handles"]["single"]
    print(f"{hd['applications_per_s']:.1f} -> {hs['applications_per_s']:.1f} applications/s (spread of the double handle over the rounds "
          f"{100 * hd['cycle_ms']['spread_rel']:.1f} %), change of one application {change:.2e}, PCG "
          f"{hd['pcg']['iterations']} / {hs['pcg']['iterations']} iterations in {hd['pcg']['ms_median']:.1f} / {hs['pcg']['ms_median']:.1f} ms, "
          f"single not slower in every round: {out['single_not_slower_in_every_round']}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({"out": out_path, "applications_per_s": [round(hd["applications_per_s"], 1), round(hs["applications_per_s"], 1)],
                      "pcg_iterations": [hd["pcg"]["iterations"], hs["pcg"]["iterations"]],
                      "pcg_ms": [round(hd["pcg"]["ms_median"], 1), round(hs["pcg"]["ms_median"], 1)],
                      "device_memory_GB": [round(mem_d / 1e9, 2), round(mem_s / 1e9, 2)]}))


if __name__ == "__main__":
    main()
