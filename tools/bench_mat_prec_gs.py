#!/usr/bin/env python3
"""Single-precision images of the block Gauss-Seidel levels (mat_prec = "single_gs") against double: one process, one
hierarchy, alternating rounds.

    python tools/bench_mat_prec_gs.py [nv] --config cfg3|cfg5|cfg2 [--smoother hgs|gs] [--rounds 5] [--reps 20] [--out FILE] [--commit ID]

Builds the hierarchy of the benchmark configuration as bench.py does (fem.elasticity_fast((nv,)*3) without / with rotations,
nv = 126; SPW hierarchy, max_coarse_size 50) and one double and one single handle on it.  --smoother hgs is bench.py's "gs" (level 0
block-coloured, the coarser block levels hybrid-block; AMGX_NO_BGSB_BC=1 in the environment makes level 0 hybrid-block as well),
--smoother gs with AMGX_BGS_BSELL_MIN=1 the multicolour BSELL form.  Per handle and round: applications per second (device vectors,
graph replay, one stream), the rounds of the two handles alternating; once per handle: amgx_pcg iterations and time to 1e-8; per
level, alternating: amgx_time_op 11 (the backward block sweep inside the cycle: the `off` stream and the in-block colour phases, or
the launches per colour), 5 (the sweep from zero, `rest` / the upper residual, the restriction) and 0 (the fp64 residual, the same
kernel for both handles), the form, the float images and their value bytes, and the device memory each handle took.  Cross-run
numbers differ by several per cent between machines and processes, so only the lines of one run compare.  Needs a GPU.

--config cfg2: the scalar hierarchy of bench.py's flagship (fem.poisson_fast((nv,)*3, jitter 0.2, seed 1), nv = 215 unless
given) with mat_prec = "single_gs_all": --smoother hgs the block-hybrid form, gs the multicolour form.  The sweep inside the cycle is
amgx_time_op 9 there (op 11 is the block sweep), the report carries gs_prec_info of every level and the spread of the double handle's
rounds, and the result goes to profiles/r29/."""
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
    ap.add_argument("--config", default="cfg3", choices=["cfg3", "cfg5", "cfg2"])
    ap.add_argument("--smoother", default="hgs", choices=["hgs", "gs"])
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
        sys.exit("bench_mat_prec_gs: needs a GPU")
    from ngsamg_amd import fem, Matrix
    from ngsamg_amd.hierarchy import Hierarchy
    from ngsamg_amd.device import DeviceAMGMatrix
    from ngsamg_amd.krylov import NativeCGSolver
    from ngsamg_amd._lib import NgsAMGError
    scalar = args.config == "cfg2"
    nv = args.nv or (215 if scalar else 126)
    knobs = {k: v for k, v in os.environ.items() if k.startswith("AMGX_")}
    out_path = args.out or os.path.join(ROOT, "profiles", "r29" if scalar else "r23", f"mat_prec_gs_{args.config}_{args.smoother}.json")
    t0 = time.time()
    rot = args.config == "cfg5"
    if scalar:
        p = fem.poisson_fast((nv, nv, nv), dirichlet="right|top", jitter=0.2, seed=1)
        H = Hierarchy(Matrix(p.n, p.n, 1, 1, p.rowptr, p.col, p.val), p.free, p.coords, dim=3, energy=0, max_coarse_size=50, max_levels=10, spw=1)
    else:
        p = fem.elasticity_fast((nv, nv, nv), dirichlet="left", mu=1.0, lam=0.5, rotations=rot)
        H = Hierarchy(Matrix(p.n, p.n, p.bs, p.bs, p.rowptr, p.col, p.val), p.free, p.coords, dim=3, energy=1, max_coarse_size=50,
                      regularize_cmats=0 if rot else 1, spw=1)
    print(f"hierarchy: {[lv.n for lv in H.levels]} block sizes {[lv.bs for lv in H.levels]} ({time.time() - t0:.1f} s)", flush=True)
    n = p.n * p.bs
    free = np.repeat(p.free, p.bs).astype(np.float64)
    rng = np.random.default_rng(0)
    b = torch.from_numpy(rng.standard_normal(n) * free).cuda()
    load = b if scalar else torch.from_numpy(np.ascontiguousarray(np.asarray(p.load, dtype=np.float64).reshape(-1))).cuda()
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
        dev = DeviceAMGMatrix(H, device=0, sm_type=args.smoother, **kw)
        torch.cuda.synchronize()
        return dev, int(free0 - torch.cuda.mem_get_info()[0]), time.time() - t1

    dbl, mem_d, t_d = create()
    sgl, mem_s, t_s = create(mat_prec="single_gs_all" if scalar else "single_gs")
    handles = {"double": dbl, "single": sgl}
    print(f"handles created in {t_d:.1f} / {t_s:.1f} s, device memory {mem_d / 1e9:.2f} / {mem_s / 1e9:.2f} GB", flush=True)
    out = {"commit": args.commit or _commit(), "config": args.config, "smoother": args.smoother, "environment": knobs, "nv": nv, "n": int(n),
           "levels": [int(lv.n) for lv in H.levels], "block_sizes": [int(lv.bs) for lv in H.levels], "device": torch.cuda.get_device_name(0),
           "rounds": args.rounds, "reps": args.reps, "device_memory_bytes": {"double": mem_d, "single": mem_s}, "handles": {}}
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
        h = {"cycle_ms": {"median": statistics.median(times[k]), "min": min(times[k]), "max": max(times[k]), "rounds": times[k]},
             "applications_per_s": 1000.0 / statistics.median(times[k]), "applications_per_s_spread": [1000.0 / max(times[k]), 1000.0 / min(times[k])],
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
        h["pcg"] = {"iterations": int(cg.iterations), "converged": bool(cg.errors[-1] <= 1e-8 * cg.errors[0]), "ms_median": statistics.median(pt),
                    "ms_min": min(pt), "final_rel_err": float(cg.errors[-1] / cg.errors[0])}
        out["handles"][k] = h
    out["relative_change_of_one_application"] = change
    out["single_not_slower_in_every_round"] = all(s <= d for s, d in zip(times["single"], times["double"]))
    lv = []
    with torch.cuda.stream(stream):                            # (op 11 needs a stream that is not the default one)
        for l in range(H.n_levels - 1):
            lp, ex = sgl.level_paths(l), sgl.level_extra(l)
            e = {"level": l, "n": int(H.levels[l].n), "bs": int(H.levels[l].bs), "gs_form": lp["gs_form"], "gs_split": lp["gs_split"],
                 "gs_f32": ex["gs_f32"], "gs_f32_images": ex["gs_f32_images"], "gs_f32_value_bytes": ex["gs_f32_bytes"],
                 "A": dbl.matrix_info(l, "A"), "A32": sgl.matrix_info(l, "A32")}
            if scalar:
                e["gs_prec_info"] = sgl.gs_prec_info(l)
                e["gs_down"] = lp["gs_down"]
            # (the sweep inside the cycle: op 9 on a scalar level, op 11 on a block level; the key keeps its name)
            for op, key in ((9 if scalar else 11, "op11_backward_sweep_ms"), (5, "op5_down_ms"), (0, "op0_residual_fp64_ms")):
                t = {"double": [], "single": []}
                try:
                    for _ in range(args.rounds):               # alternating
                        for k, dev in handles.items():
                            t[k].append(dev.time_op(l, op, args.op_reps))
                except NgsAMGError as err:                     # (a collapsed level, a level without a block sweep)
                    e[key] = {"unmeasured": str(err)}
                    continue
                e[key] = {k: statistics.median(v) for k, v in t.items()}
                e[key]["single_over_double"] = e[key]["single"] / e[key]["double"]
            lv.append(e)

            def fmt(key):
                v = e[key]
                return "-" if "unmeasured" in v else f"{v['double']:.4f} -> {v['single']:.4f} ms ({v['single_over_double']:.2f})"
            print(f"  level {l}: n {e['n']} bs {e['bs']} {e['gs_form']} split {e['gs_split']} f32 {e['gs_f32']} ({e['gs_f32_images']} images, "
                  f"{e['gs_f32_value_bytes']} B)  op11 {fmt('op11_backward_sweep_ms')}  op5 {fmt('op5_down_ms')}  op0 {fmt('op0_residual_fp64_ms')}", flush=True)
    out["per_level"] = lv
    hd, hs = out["handles"]["double"], out["handles"]["single"]
    sp = hd["applications_per_s_spread"]
    print(f"{hd['applications_per_s']:.1f} (rounds {sp[0]:.1f} ... {sp[1]:.1f}) -> {hs['applications_per_s']:.1f} applications/s, change of one application {change:.2e}, PCG "
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
