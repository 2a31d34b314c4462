#!/usr/bin/env python
"""Times amgx_mv_gram and amgx_mv_combine on device tensors against torch.matmul on the same tensors, in the same process, in
alternating rounds; optionally the block eigensolver at a bench.py configuration.

    python tools/bench_mv.py                                   # n = 9 938 375 (cfg 2), k = 4, 8, 24, both layouts
    python tools/bench_mv.py --eigen --config cfg2 --smoother cheby|jacobi

Byte models: Gram 8 n (ka + kb), 8 n ka when A is B; combine 8 n (kx + ky (1 + [beta != 0])).
torch.matmul is what a user could call today, hence the yardstick: ratio = our time / torch's time (below 1: faster).
Gram calls are timed with a host clock around call + result on the host (both sides: the caller needs G there); combine calls
with device events around `reps` enqueued calls.  One JSON line per measurement, a table at the end.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def small_handle():
    from ngsamg_amd import fem
    from ngsamg_amd._lib import Matrix
    from ngsamg_amd.hierarchy import Hierarchy
    from ngsamg_amd.device import DeviceAMGMatrix
    p = fem.poisson_fast((9, 9), dirichlet="left|top")
    H = Hierarchy(Matrix(p.n, p.n, 1, 1, p.rowptr, p.col, p.val), p.free, p.coords, dim=2, energy=0, max_coarse_size=5)
    return DeviceAMGMatrix(H, sm_type="jacobi")


def host_time(fn, reps):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def event_time(fn, reps):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def alternate(ours, theirs, timer, reps, rounds):
    """median of `rounds` alternating measurements of each side (one untimed warm-up each)"""
    ours(), theirs()
    a, b = [], []
    for _ in range(rounds):
        a.append(timer(ours, reps))
        b.append(timer(theirs, reps))
    return statistics.median(a), statistics.median(b), (min(a), max(a)), (min(b), max(b))


def primitives(args):
    import torch
    from ngsamg_amd import _lib
    dev = small_handle()
    lib, h = dev._lib, dev._h
    n = args.n
    rows = []
    rng = np.random.default_rng(0)
    for k in args.k:
        for il in (False, True):
            shape = (n, k) if il else (k, n)
            A = torch.randn(shape, dtype=torch.float64, device="cuda")
            B = torch.randn(shape, dtype=torch.float64, device="cuda")
            Y = torch.randn(shape, dtype=torch.float64, device="cuda")
            flags = dev._multi_flags(True, il)
            G = np.empty((k, k))
            pg = _lib.ptr(G, C.c_double)
            for sym in (True, False):
                Bx = A if sym else B

                def ours():
                    dev._ck(lib.amgx_mv_gram(h, n, k, A.data_ptr(), n, k, Bx.data_ptr(), n, pg, flags))

                def theirs():
                    return (torch.matmul(A.T, Bx) if il else torch.matmul(A, Bx.T)).cpu()
                t, tt, sp, spt = alternate(ours, theirs, host_time, args.reps, args.rounds)
                nbytes = 8 * n * (k if sym else 2 * k)
                rows.append(dict(op="gram", form="A^T A" if sym else "A^T B", k=k, layout="interleaved" if il else "column-major", ms=t,
                                 gbs=nbytes / t / 1e6, torch_ms=tt, ratio=t / tt, spread=sp, torch_spread=spt))
                print(json.dumps(rows[-1]), flush=True)
            for kx, ky in ((k, k), (24, 8)) if k == 8 else ((k, k),):
                X = A if kx == k else torch.randn((n, kx) if il else (kx, n), dtype=torch.float64, device="cuda")
                Yk = Y if ky == k else torch.randn((n, ky) if il else (ky, n), dtype=torch.float64, device="cuda")
                c = np.ascontiguousarray(rng.standard_normal((kx, ky)))
                pc = _lib.ptr(c, C.c_double)
                cd = torch.from_numpy(c).cuda()
                cdT = cd.T.contiguous()
                for beta in (0.0, 1.0):
                    def ours():
                        dev._ck(lib.amgx_mv_combine(h, n, kx, X.data_ptr(), n, pc, ky, beta, Yk.data_ptr(), n, flags))

                    def theirs():
                        if il:
                            return torch.matmul(X, cd, out=Yk) if beta == 0.0 else torch.addmm(Yk, X, cd, beta=beta, out=Yk)
                        return torch.matmul(cdT, X, out=Yk) if beta == 0.0 else torch.addmm(Yk, cdT, X, beta=beta, out=Yk)
                    Yk.normal_()
                    t, tt, sp, spt = alternate(ours, theirs, event_time, args.reps, args.rounds)
                    nbytes = 8 * n * (kx + ky * (2 if beta != 0.0 else 1))
                    rows.append(dict(op="combine", form=f"{kx}->{ky} beta={beta:g}", k=k, layout="interleaved" if il else "column-major",
                                     ms=t, gbs=nbytes / t / 1e6, torch_ms=tt, ratio=t / tt, spread=sp, torch_spread=spt))
                    print(json.dumps(rows[-1]), flush=True)
            del A, B, Y
            torch.cuda.empty_cache()
    print(f"\nn = {n}, reps {args.reps}, median of {args.rounds} alternating rounds; GB/s against the byte model")
    print(f"{'op':8s} {'form':16s} {'k':>3s} {'layout':13s} {'ms':>8s} {'GB/s':>8s} {'torch ms':>9s} {'ratio':>6s}")
    for r in rows:
        print(f"{r['op']:8s} {r['form']:16s} {r['k']:3d} {r['layout']:13s} {r['ms']:8.3f} {r['gbs']:8.0f} {r['torch_ms']:9.3f} {r['ratio']:6.2f}")


def eigen(args):
    import torch
    from ngsamg_amd import fem
    from ngsamg_amd._lib import Matrix
    from ngsamg_amd.hierarchy import Hierarchy
    from ngsamg_amd.device import DeviceAMGMatrix
    from ngsamg_amd.eigen import lobpcg
    from ngsamg_amd.multivector import DeviceMultiVector, MatVecMulti, MultMulti
    if args.config != "cfg2":
        raise SystemExit("bench_mv.py --eigen: only cfg2 is set up here")
    nv = args.nv
    t0 = time.time()
    prob = fem.poisson_fast((nv, nv, nv), dirichlet="right|top", jitter=0.2, seed=1)
    H = Hierarchy(Matrix(prob.n, prob.n, 1, 1, prob.rowptr, prob.col, prob.val), prob.free, prob.coords, dim=3, energy=0,
                  max_coarse_size=50, max_levels=10, spw=1)
    dev = DeviceAMGMatrix(H, sm_type=args.smoother, omega=0.9)
    print(f"cfg2: {nv}^3 = {prob.n} dofs, {H.n_levels} levels, smoother {args.smoother}, setup {time.time() - t0:.1f} s", flush=True)
    free = torch.from_numpy(prob.free.astype(np.float64)).cuda()
    for num in (4, 8):
        for fuse in (False, True):
            plan = dev.multi_plan(num, fuse=fuse)
            for history in (True, False):
                X0 = DeviceMultiVector(dev, torch.from_numpy(np.random.default_rng(1).standard_normal((num, prob.n))).cuda())
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                lams, X, info = lobpcg(MatVecMulti(0, dev), MultMulti(dev), num, free=free, X0=X0, tol=args.tol, maxit=args.maxit,
                                       history=history, fuse=fuse)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                print(json.dumps(dict(op="lobpcg" if history else "pinvit", num=num, fuse=fuse, fused=plan["fused"], groups=plan["groups"],
                                      smoother=args.smoother, seconds=dt, iterations=int(info["iterations"]), status=info["status"],
                                      ms_per_iteration=1e3 * dt / max(1, info["iterations"]), pre_columns=info["pre_columns"],
                                      lams=[float(v) for v in lams], max_res=float(np.max(info["res"][-1])))), flush=True)
                del X0, X
                torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=9938375, help="rows (default: 215^3, the cfg-2 size)")
    ap.add_argument("--k", type=int, nargs="+", default=[4, 8, 24])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--eigen", action="store_true", help="time lobpcg (4 and 8 pairs, fuse off / on) instead of the primitives")
    ap.add_argument("--config", default="cfg2")
    ap.add_argument("--smoother", default="jacobi", choices=["jacobi", "cheby"])
    ap.add_argument("--nv", type=int, default=215)
    ap.add_argument("--tol", type=float, default=1e-8)
    ap.add_argument("--maxit", type=int, default=100)
    args = ap.parse_args()
    (eigen if args.eigen else primitives)(args)


if __name__ == "__main__":
    main()
