#!/usr/bin/env python3
"""Wall time of amgx_create for the block-hybrid Gauss-Seidel hierarchy of a bench.py configuration, for A/B runs of two builds of
the device library (NGSAMG_HIP_LIB selects the other build; one process per library, alternate them as tools/ab_libs.sh does):

  python tools/setup_ab.py --config cfg2|cfg3 [--nv N] [--repeat 3]

The host hierarchy is built once; DeviceAMGMatrix(H, sm_type="hgs") is then constructed --repeat times (the first one also loads
the code objects) and one cycle is applied.  Prints one line: the create times in seconds and the norm of the cycle's result."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg2", choices=["cfg2", "cfg3"])
    ap.add_argument("--nv", type=int, default=None)
    ap.add_argument("--repeat", type=int, default=3)
    a = ap.parse_args()
    import numpy as np
    import torch
    from ngsamg_amd import fem
    from ngsamg_amd._lib import Matrix
    from ngsamg_amd.device import DeviceAMGMatrix
    from ngsamg_amd.hierarchy import Hierarchy
    nv = a.nv or (215 if a.config == "cfg2" else 126)
    if a.config == "cfg2":                    # (the hierarchies of bench.py)
        p = fem.poisson_fast((nv, nv, nv), dirichlet="right|top", jitter=0.2, seed=1)
        H = Hierarchy(Matrix(p.n, p.n, 1, 1, p.rowptr, p.col, p.val), p.free, p.coords, dim=3, energy=0, max_coarse_size=50, max_levels=10, spw=1)
    else:
        p = fem.elasticity_fast((nv, nv, nv), dirichlet="left", mu=1.0, lam=0.5, rotations=False)
        H = Hierarchy(Matrix(p.n, p.n, p.bs, p.bs, p.rowptr, p.col, p.val), p.free, p.coords, dim=3, energy=1, max_coarse_size=50, regularize_cmats=1, spw=1)
    times = []
    for _ in range(a.repeat):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dev = DeviceAMGMatrix(H, sm_type="hgs", device=0)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
        forms = [dev.level_paths(l)["gs_form"] for l in range(dev.n_levels)]
        if len(times) < a.repeat:
            del dev
    n = p.n * p.bs
    b = torch.from_numpy(np.random.default_rng(0).standard_normal(n) * np.repeat(p.free, p.bs)).cuda()
    x = torch.empty_like(b)
    dev.Mult(b, x)
    torch.cuda.synchronize()
    lib = os.environ.get("NGSAMG_HIP_LIB", "tree")
    print(f"{a.config} nv={nv} lib={os.path.basename(lib)} amgx_create s: " + " ".join(f"{t:.3f}" for t in times) +
          f"  x_norm {float(torch.linalg.norm(x)):.10e}  forms {' '.join(forms)}", flush=True)


if __name__ == "__main__":
    main()
