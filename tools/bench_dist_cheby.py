#!/usr/bin/env python3
"""Cost of the rank-partitioned Chebyshev cycle next to the rank-partitioned Jacobi cycles, on one GPU.

  python tools/bench_dist_cheby.py [--nv 108] [--rounds 3] [--reps 30] [--out FILE.json]

Two transports: "loopback" = 2 virtual ranks (LoopbackComm) of nv^3 vertices each, whose kernels serialise on the one device, and
"rccl1" = a real RCCL communicator at world size 1 with nv^3 vertices.  Four configurations: Jacobi in the literal stage order,
Jacobi folded, Chebyshev degree 1 and degree 2.  Per configuration: ms per Mult (whole-cycle graph replay, a host clock around
`reps` applications that end in a device synchronise, after warm-up) and PCG iterations / seconds to 1e-8.

Every (transport, configuration) runs in a process of its own; the rounds alternate over the configurations, so a drift of the
box hits all of them alike.  Reported: the median over the rounds and the spread (min .. max).  What this cannot show is the
wire: between virtual ranks an exchange is a device copy, at world size 1 there is no peer."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {"jacobi literal": dict(sm_type="jacobi", fold=False), "jacobi folded": dict(sm_type="jacobi", fold=True),
           "cheby degree 1": dict(sm_type="cheby", cheb_degree=1), "cheby degree 2": dict(sm_type="cheby", cheb_degree=2)}


def child(a):
    import torch
    from ngsamg_amd import dist as D
    nv = a.nv
    if a.transport == "rccl1":
        import torch.distributed as dist
        torch.cuda.set_device(0)
        dist.init_process_group("gloo", rank=0, world_size=1)
        comm, pg, R = D.TorchComm(), (1, 1, 1), 1
    else:
        comm, pg, R = D.LoopbackComm(2), (2, 1, 1), 2
    t0 = time.perf_counter()
    ranks = range(R) if a.transport == "loopback" else [0]
    states = [D.assemble_poisson_owned(r, pg, (nv, nv, nv)) for r in ranks]
    amg = D.DistributedAMG(comm, states, dim=3, dist_min_rows=50000, device=0, max_coarse_size=50, **CONFIGS[a.config])
    setup = time.perf_counter() - t0
    rng = np.random.default_rng(0)
    bs = [torch.from_numpy(rng.standard_normal(s.n) * s.free).cuda() for s in states]
    xs = [torch.zeros_like(b) for b in bs]
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        e0 = amg._dev.n_exchanges()
        amg.Mult(bs, xs)
        per_cycle = amg._dev.n_exchanges() - e0
        for _ in range(5):
            amg.Mult(bs, xs)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.reps):
            amg.Mult(bs, xs)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / a.reps * 1e3
        xk = [torch.zeros_like(b) for b in bs]
        amg.pcg(bs, xk, tol=1e-8, maxsteps=200)              # warm-up: workspace, the preconditioner's graph on these vectors
        for x in xk:
            x.zero_()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        it, errs = amg.pcg(bs, xk, tol=1e-8, maxsteps=200)
        torch.cuda.synchronize()
        pcg_s = time.perf_counter() - t0
    gi = amg._dev.graph_info()
    out = dict(transport=a.transport, config=a.config, nv=nv, ranks=R, rows_per_rank=[int(s.n) for s in states], dist_levels=int(amg.k),
               level_rows=[[int(lv[i].n) for i in range(len(states))] for lv in amg.dist_levels], setup_s=setup, ms_per_mult=ms,
               exchanges_per_mult=int(per_cycle), pcg_iterations=int(it), pcg_seconds=pcg_s, pcg_final_rel=float(errs[-1] / errs[0]),
               graph=gi["enabled"], graph_replays=int(gi["replays"]))
    if CONFIGS[a.config]["sm_type"] == "cheby":
        out["lambda_max"] = [amg.smoother_info(l)["lambda_max"] for l in range(amg.k)]
    print("RESULT " + json.dumps(out), flush=True)
    if a.transport == "rccl1":
        dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nv", type=int, default=108)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out")
    ap.add_argument("--transport")
    ap.add_argument("--config")
    a = ap.parse_args()
    if a.config:
        return child(a)
    import socket
    runs = []
    for rnd in range(a.rounds):
        for transport in ("loopback", "rccl1"):
            for config in CONFIGS:
                env = dict(os.environ)
                if transport == "rccl1":
                    with socket.socket() as s:
                        s.bind(("127.0.0.1", 0))
                        port = s.getsockname()[1]
                    env.update(RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--nv", str(a.nv), "--reps", str(a.reps), "--transport", transport,
                                    "--config", config], env=env, capture_output=True, text=True, timeout=600)
                line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
                if r.returncode != 0 or not line:       # nothing more is started on the GPU after a child that failed
                    sys.exit(f"{transport} / {config} ended with status {r.returncode}:\n{r.stdout[-2000:]}{r.stderr[-2000:]}")
                runs.append(dict(json.loads(line[0][7:]), round=rnd))
                print(f"round {rnd} {transport:8s} {config:15s} {runs[-1]['ms_per_mult']:8.3f} ms / Mult   pcg {runs[-1]['pcg_iterations']:3d} it "
                      f"{runs[-1]['pcg_seconds'] * 1e3:8.1f} ms   exchanges / Mult {runs[-1]['exchanges_per_mult']}", flush=True)
    summary = []
    for transport in ("loopback", "rccl1"):
        for config in CONFIGS:
            rs = [r for r in runs if r["transport"] == transport and r["config"] == config]
            ms, ps = [r["ms_per_mult"] for r in rs], [r["pcg_seconds"] for r in rs]
            summary.append(dict(transport=transport, config=config, ms_per_mult_median=statistics.median(ms), ms_per_mult_min=min(ms),
                                ms_per_mult_max=max(ms), pcg_iterations=rs[0]["pcg_iterations"], pcg_seconds_median=statistics.median(ps),
                                pcg_seconds_min=min(ps), pcg_seconds_max=max(ps), exchanges_per_mult=rs[0]["exchanges_per_mult"]))
    print("\ntransport config            ms / Mult median (min .. max)     pcg it   pcg s median (min .. max)   exchanges / Mult")
    for s in summary:
        print(f"{s['transport']:9s} {s['config']:15s} {s['ms_per_mult_median']:8.3f} ({s['ms_per_mult_min']:.3f} .. {s['ms_per_mult_max']:.3f})   "
              f"{s['pcg_iterations']:6d}   {s['pcg_seconds_median']:.4f} ({s['pcg_seconds_min']:.4f} .. {s['pcg_seconds_max']:.4f})   {s['exchanges_per_mult']}")
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(nv=a.nv, rounds=a.rounds, reps=a.reps, summary=summary, runs=runs), f, indent=1)


if __name__ == "__main__":
    main()
