#!/usr/bin/env python3
"""Chebyshev smoother on a rank-partitioned hierarchy over a real RCCL communicator at world size 1, through the C ABI
(amgx_comm_* / amgx_dist_*), checked against tests/cheby_ref.py::ChebyRef on the assembled global hierarchy.

    python tests/dist_rccl_cheby_check.py [--box B] [--degree D] [--dmin N]

Modelled on tests/dist_rccl_check.py: without RANK in the environment the script starts the rank itself (a fresh child process,
before any GPU call) under the rank watchdog of bench.py and relays its verdict.  What runs: ncclCommInitRank, the collective
lambda_max estimate (amgx_dist_cheb_estimate), three applications (direct launches, capture, replay) of the overlapped Chebyshev
driver and the all-gather of level k."""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--box", type=int, default=20)
    ap.add_argument("--degree", type=int, default=2)
    ap.add_argument("--dmin", type=int, default=500)
    return ap.parse_args()


def launch():
    import signal
    import socket
    import bench                       # the rank watchdog is the one bench.py --gpus N uses
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []

    def reap(*_):
        for p in procs:
            if p.poll() is None:
                p.kill()

    signal.signal(signal.SIGTERM, lambda *a: (reap(), sys.exit(143)))
    try:
        env = dict(os.environ, RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env, start_new_session=True,
                                      stdout=subprocess.PIPE, text=True))
        codes, out, why = bench._wait_ranks(procs, float(os.environ.get("NGSAMG_CHECK_TIMEOUT", "300")))
    finally:
        reap()
    sys.stdout.write(out or "")
    if why:
        print("stopped:", why)
    print("exit codes", codes)
    sys.exit(0 if all(c == 0 for c in codes) and not why else 1)


def main():
    args = parse()
    if "RANK" not in os.environ:
        launch()
    import torch
    import torch.distributed as dist
    from ngsamg_amd import dist as D
    from tests.cheby_ref import ChebyRef
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=0, world_size=1)
    code = 1
    try:
        st = D.assemble_poisson_owned(0, (1, 1, 1), (args.box,) * 3)
        amg = D.DistributedAMG(D.TorchComm(), [st], dim=3, dist_min_rows=args.dmin, device=0, max_coarse_size=20, sm_type="cheby",
                               cheb_degree=args.degree)
        infos = [amg.smoother_info(l) for l in range(amg.k)]
        rng = np.random.default_rng(0)
        bh = rng.standard_normal(st.n) * st.free
        b = torch.from_numpy(bh).to("cuda:0")
        x = torch.full_like(b, float("nan"))
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            for _ in range(3):
                amg.Mult([b], [x])
        torch.cuda.synchronize()
        gi = amg._dev.graph_info()
        glv = amg.global_levels()
        lam = [amg.smoother_info(l)["lambda_max"] if l + 1 < len(glv) else 1.0 for l in range(len(glv))]
        n = int(amg.tail_hier.coarse_n)
        cinv = np.asarray(amg.tail_hier.coarse_inv, dtype=np.float64).reshape(n, n) if n else None
        ref = ChebyRef(glv, sm="cheby", degree=args.degree, lambda_max=lam, coarse_inv=cinv).apply(bh)
        err = float(np.linalg.norm(x.cpu().numpy() - ref) / np.linalg.norm(ref))
        est = min(i["estimated"] for i in infos)
        print(f"world=1 box={args.box}^3 degree={args.degree} distributed levels={amg.k} estimated = {est} "
              f"lambda_max = {[i['lambda_max'] for i in infos]} rel.err vs ChebyRef = {err:.3e} "
              f"graph enabled = {gi['enabled']} graphs = {gi['graphs']} replays = {gi['replays']} note = '{gi['note']}'")
        ok = err <= 1e-12 and est == 1
        print("RCCL CHEBY CHECK", "PASSED" if ok else "FAILED")
        code = 0 if ok else 1
    finally:
        dist.destroy_process_group()
    sys.exit(code)


if __name__ == "__main__":
    main()
