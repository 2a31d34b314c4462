#!/usr/bin/env python3
"""Bits against another build of the device library: the same (handle, call) cases in a fresh child process per library -- first
the tree's own build, then NGSAMG_HIP_LIB=<other build>, usually the parent commit's -- every result stored as .npy and compared
with numpy.array_equal, level_paths(l) of every level of every handle compared as dictionaries.  Prints the table and a verdict.

  python tools/bits_vs_parent.py --parent-lib <libngsamg_hip.so of the parent> --out <dir> [--report <file>] [--parent-root <dir>]
                                 [--cases single,dist,multi]

--parent-root: a built checkout of the parent commit; its own copy of this tool (hence its Python package) then drives the parent's
library -- needed whenever this tree's bindings name an entry point the parent's library does not have.

The cases are the Gauss-Seidel forms (every SweepPath value, with and without the split images where a kill switch exists) and
the rank-partitioned drivers on two virtual ranks, and the four multi-vector entries under every fuse word with the answers of
multi_plan / multi_level_plan (MULTI_CASES: every Gauss-Seidel form that has sweeps on 2 and 4 vectors, each on a handle that must run
fused groups under its fuse word in both builds); edit CASES / DIST_CASES / MULTI_CASES for the refactor at hand.  A child that fails
ends the run: nothing more is started on the GPU after it."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FLAGS = ((False, False, False), (False, True, False), (True, True, True), (False, False, True))     # res_updated, update_res, x_zero
BC = {"AMGX_BGSB_BC_MIN_ROWS": "0", "AMGX_BGSB_BC_MIN_WG": "0"}


# ---- single rank: name, problem, DeviceAMGMatrix arguments, environment at create
def _poisson(shape):
    from tests.problems import poisson_case
    p, H = poisson_case(shape)
    return H, p.free, 1


def _poisson_blocks(shape):
    H, free, bs = _poisson(shape)
    H.build_bgs()                                      # (aggregate blocks for sm_type "bgs")
    return H, free, bs


def _elasticity(shape):
    from tests.problems import elasticity_case
    p, H = elasticity_case(shape, rotations=False, max_coarse_size=10)
    return H, p.free, p.bs


def _scalar_rows(L, l1=False):
    import numpy as np
    from tests import reorder as R
    A, B, free, H = R.gs_scalar_case(L, "identity")
    if l1:
        free = np.ones(A.shape[0], np.uint8)
        H = R.gs_hierarchy(A, free, l1_dinv=True, seed=L)
    return H, free, 1


def _block_rows(bs, L=151, n=None, odd=False):
    import numpy as np
    from tests import reorder as R
    n = n or {2: 700, 3: 500, 6: 400}[bs]
    A = R.block_long_row_matrix(bs, L, n, seed=bs + L, odd_only=odd)
    free = np.ones(n, np.uint8)
    free[np.random.default_rng(bs).choice(n, size=7, replace=False)] = 0
    return R.gs_hierarchy(A, free, bs=bs, seed=bs), free, bs


CYCLES = [dict(mg_cycle="W"), dict(mg_cycle="BS"), dict(sm_steps=2), dict(sm_symm=True)]
CASES = []
for split in (True, False):
    off = {} if split else {"AMGX_GSB_NO_SPLIT": "1"}
    tag = "split" if split else "no split"
    CASES += [(f"hybrid scalar 21^3 {tag}", (_poisson, (21, 21, 21)), dict(sm_type="hgs"), off, True),
              (f"hybrid scalar rows of 64 {tag}", (_scalar_rows, 64), dict(sm_type="hgs"), off, True)]
    CASES += [(f"hybrid scalar 21^3 {tag} {kw}", (_poisson, (21, 21, 21)), dict(sm_type="hgs", **kw), off, False) for kw in CYCLES]
    off = {} if split else {"AMGX_BGSB_NO_SPLIT": "1"}
    CASES += [(f"hybrid block bs=3 {tag}", (_block_rows, 3), dict(sm_type="hgs"), off, True),
              (f"block-coloured bs=3 {tag}", (_block_rows, 3), dict(sm_type="hgs"), {**off, **BC}, True),
              (f"block-coloured elasticity 14x13x12 {tag}", (_elasticity, (14, 13, 12)), dict(sm_type="hgs"), {**off, **BC}, True)]
    CASES += [(f"hybrid block elasticity 14x13x12 {tag} {kw}", (_elasticity, (14, 13, 12)), dict(sm_type="hgs", **kw), off, False)
              for kw in [{}] + CYCLES]
    off = {} if split else {"AMGX_NO_BGS_SPLIT": "1"}
    CASES += [(f"multicolour bsell bs=3 {tag}", (_block_rows, 3, 151, None, True), dict(sm_type="gs"), {"AMGX_BGS_BSELL_MIN": "1", **off}, True)]
CASES += [("multicolour scalar 21^3 split", (_poisson, (21, 21, 21)), dict(sm_type="gs"), {}, True),
          ("multicolour scalar rows of 15 split", (_scalar_rows, 15), dict(sm_type="gs"), {}, True),
          ("multicolour scalar rows of 15 l1 diagonal, no split", (_scalar_rows, 15, True), dict(sm_type="gs"), {}, True),
          ("multicolour row list bs=2", (_block_rows, 2, 17, 700), dict(sm_type="gs"), {"AMGX_NO_BGS_BSELL": "1"}, True),
          ("aggregate blocks 14x13x12", (_poisson_blocks, (14, 13, 12)), dict(sm_type="bgs"), {}, True),
          ("jacobi 21^3", (_poisson, (21, 21, 21)), dict(sm_type="jacobi"), {}, False)]
# both image builders of the Gauss-Seidel data: the host loops (small levels, above) and the device kernels (DEV: every level)
DEV = {"AMGX_DEV_IMAGES_MIN_ROWS": "0"}
DEV1 = {**DEV, "AMGX_SELL_MAX_LANES": "1"}            # scalar levels: the device builder forms the one-lane images only
COMPACT = {"AMGX_BGSB_COMPACT": "1"}
LW = {"AMGX_GSB_LW": "1", "AMGX_LW_MIN_ROWS": "0"}
CASES += [("hybrid scalar 21^3 device images", (_poisson, (21, 21, 21)), dict(sm_type="hgs"), DEV1, True),
          ("hybrid scalar rows of 64 device images", (_scalar_rows, 64), dict(sm_type="hgs"), DEV1, True),
          ("hybrid block bs=3 device images", (_block_rows, 3), dict(sm_type="hgs"), DEV, True),
          ("block-coloured bs=3 device images", (_block_rows, 3), dict(sm_type="hgs"), {**BC, **DEV}, True),
          ("compact blocks bs=3", (_block_rows, 3), dict(sm_type="hgs"), COMPACT, True),
          ("compact blocks bs=3 device images", (_block_rows, 3), dict(sm_type="hgs"), {**COMPACT, **DEV}, True),
          ("hybrid scalar rows of 64 local window", (_scalar_rows, 64), dict(sm_type="hgs"), LW, True),
          ("hybrid scalar rows of 64 local window device images", (_scalar_rows, 64), dict(sm_type="hgs"), {**LW, **DEV1}, True),
          ("multicolour bsell bs=2 split", (_block_rows, 2, 151, None, True), dict(sm_type="gs"), {"AMGX_BGS_BSELL_MIN": "1"}, True)]

# ---- two virtual ranks: name, problem, DistributedAMG arguments, environment at create
HGS = dict(sm_type="hgs", hgs_block_rows=256)
ELAST = dict(dist_min_rows=150, max_coarse_size=5, energy=1, regularize_cmats=1, sm_type="hgs", hgs_block_rows=42)
STEPS = [dict(sm_steps=2, mg_cycle="V"), dict(mg_cycle="W")]
DIST_CASES = [("dist hybrid scalar split", "poisson", dict(dist_min_rows=200, **HGS), {}),
              ("dist hybrid scalar no split", "poisson", dict(dist_min_rows=200, **HGS), {"AMGX_GSB_NO_SPLIT": "1"}),
              ("dist hybrid block split", "elasticity", ELAST, {}),
              ("dist hybrid block no split", "elasticity", ELAST, {"AMGX_BGSB_NO_SPLIT": "1"}),
              ("dist staged gs", "poisson", dict(dist_min_rows=200, sm_type="gs", gs_stage_min_rows=50), {}),
              ("dist staged bgs", "poisson", dict(dist_min_rows=200, sm_type="bgs"), {}),
              ("dist rank without rows hgs", "empty-rank", dict(dist_min_rows=60, gs_stage_min_rows=50, **HGS), {})]
for kw in STEPS:
    DIST_CASES += [(f"dist stepwise {sm} {kw}", "poisson", dict(dist_min_rows=200, **({"sm_type": sm} if sm != "hgs" else HGS), **kw), {})
                   for sm in ("jacobi", "hgs", "gs", "bgs")]
    DIST_CASES += [(f"dist stepwise hybrid block {kw}", "elasticity", dict(ELAST, **kw), {})]


# ---- the multi-vector entries (MultMulti, MatVecMulti, SmoothMulti, DownMulti) under every fuse word, and what multi_plan /
# multi_level_plan answer (notes and work_bytes included): name, problem, DeviceAMGMatrix arguments, environment at create
NO_DENSE = {"AMGX_NO_DENSE_TAIL": "1"}
FUSE_WORDS = (False, True, "gs", "gs_block", "down", "gs+down", "gs_block+down", "down_dia", "gs+down_dia", "gs_block+down_dia")
# last entry: the fuse word under which the handle has to run fused groups in BOTH builds (None: no such demand) -- a Gauss-Seidel
# case that stayed in the column loop would compare the single-vector sweeps with themselves
MULTI_CASES = [("multi jacobi 17^3", (_poisson, (17, 17, 17)), dict(sm_type="jacobi"), NO_DENSE, None),
               ("multi cheby 17^3", (_poisson, (17, 17, 17)), dict(sm_type="cheby", cheb_degree=2, cheb_lambda_max=2.0), NO_DENSE, None),
               ("multi hybrid scalar 17^3", (_poisson, (17, 17, 17)), dict(sm_type="hgs"), NO_DENSE, "gs"),
               ("multi hybrid block elasticity 9x8x7", (_elasticity, (9, 8, 7)), dict(sm_type="hgs"), NO_DENSE, "gs_block")]
# every other Gauss-Seidel form that has sweeps on 2 and 4 vectors (shapes and environments of tests/test_gpu_multi_gs.py and
# tests/test_gpu_multi_gs_block.py)
BSELL1 = {"AMGX_BGS_BSELL_MIN": "1"}
MULTI_CASES += [
    ("multi multicolour scalar 21^3", (_poisson, (21, 21, 21)), dict(sm_type="gs"), NO_DENSE, "gs"),
    ("multi multicolour scalar rows of 15 l1 diagonal, no split", (_scalar_rows, 15, True), dict(sm_type="gs"), NO_DENSE, "gs"),
    ("multi hybrid scalar 21^3 no split", (_poisson, (21, 21, 21)), dict(sm_type="hgs"), {**NO_DENSE, "AMGX_GSB_NO_SPLIT": "1"}, "gs"),
    ("multi hybrid scalar 21^3 512 threads", (_poisson, (21, 21, 21)), dict(sm_type="hgs"), {**NO_DENSE, "AMGX_GSB_THREADS": "512"}, "gs"),
    ("multi hybrid scalar 33x30x28 1024 threads", (_poisson, (33, 30, 28)), dict(sm_type="hgs"), {**NO_DENSE, "AMGX_GSB_THREADS": "1024"}, "gs"),
    ("multi multicolour bsell elasticity 9x8x7", (_elasticity, (9, 8, 7)), dict(sm_type="gs"), {**NO_DENSE, **BSELL1}, "gs_block"),
    ("multi multicolour bsell elasticity 9x8x7 no split", (_elasticity, (9, 8, 7)), dict(sm_type="gs"), {**NO_DENSE, **BSELL1, "AMGX_NO_BGS_SPLIT": "1"}, "gs_block"),
    ("multi multicolour row list elasticity 9x8x7", (_elasticity, (9, 8, 7)), dict(sm_type="gs"), NO_DENSE, "gs_block"),
    ("multi block-coloured elasticity 9x8x7", (_elasticity, (9, 8, 7)), dict(sm_type="hgs"), {**NO_DENSE, **BC}, "gs_block"),
    ("multi block-coloured elasticity 9x8x7 no split", (_elasticity, (9, 8, 7)), dict(sm_type="hgs"), {**NO_DENSE, **BC, "AMGX_BGSB_NO_SPLIT": "1"}, "gs_block"),
    ("multi hybrid block elasticity 9x8x7 no split", (_elasticity, (9, 8, 7)), dict(sm_type="hgs"), {**NO_DENSE, "AMGX_BGSB_NO_SPLIT": "1"}, "gs_block")]
# k = 7: groups 4 + 2 + 1; k = 4: one group, used in place when interleaved.  (k, interleaved, device tensors)
MULTI_SHAPES = ((7, False, True), (4, True, True), (7, True, False), (4, False, False))


class _Env:
    def __init__(self, env):
        self.env = env

    def __enter__(self):
        os.environ.update(self.env)

    def __exit__(self, *a):
        for k in self.env:
            del os.environ[k]


def _single(store):
    import numpy as np
    from ngsamg_amd.device import DeviceAMGMatrix
    paths = {}
    for name, (make, *args), kw, env, smooth in CASES:
        print(name, flush=True)
        H, free, bs = make(*args)
        with _Env(env):
            dev = DeviceAMGMatrix(H, device=0, **kw)
        paths[name] = [dev.level_paths(l) for l in range(dev.n_levels)]
        fr = np.repeat(np.asarray(free) > 0, bs).astype(np.float64)
        n = fr.size
        rng = np.random.default_rng(7)
        b = rng.standard_normal(n) * fr
        for rep, graph in enumerate((True, True, False)):            # capture, replay, direct launches
            x = np.full(n, np.nan)
            dev.Mult(b, x, graph=graph)
            if rep:
                store(f"{name}|Mult graph={graph}", x)
        if not smooth:
            continue
        A0 = H.levels[0].A.to_scipy()
        for back in (False, True):
            for ru, ur, xz in FLAGS:
                x = np.zeros(n) if xz else rng.standard_normal(n) * fr
                r = b - A0 @ x if ru else rng.standard_normal(n)
                dev.Smooth(0, x, b, r, ru, ur, xz, back=back)
                store(f"{name}|Smooth back={back} ru={ru} ur={ur} xz={xz}", np.concatenate([x, r]))
    return paths


def _dist_states(kind):
    import numpy as np
    from ngsamg_amd import dist as D
    if kind == "poisson":
        return D.LoopbackComm(2), [D.assemble_poisson_owned(r, D.proc_grid(2, 3), (16, 16, 16)) for r in range(2)], 1
    if kind == "elasticity":
        st = [D.assemble_elasticity_owned(r, D.proc_grid(2, 3), (12, 9, 9), rotations=False) for r in range(2)]
        return D.LoopbackComm(2), st, st[0].bs
    import scipy.sparse as sp
    from ngsamg_amd import bridge as B
    locs = []
    for r in range(4):                               # four ranks with rows behind one that owns nothing
        L, _ = B.shared_poisson_partition(r, (2, 2, 1), (17, 17, 9))
        L.rank = r + 1
        L.dist_procs = [np.asarray(p) + 1 for p in L.dist_procs]
        locs.append(L)
    empty = B.SharedLocal(0, sp.csr_matrix((0, 0)), [], free=np.zeros(0, dtype=np.uint8), coords=np.zeros((0, 3)))
    comm = D.LoopbackComm(5)
    return comm, B.from_shared_layout(comm, [empty] + locs)[0], 1


def _dist(store):
    import numpy as np
    import torch
    from ngsamg_amd import dist as D
    paths = {}
    for name, kind, kw, env in DIST_CASES:
        print(name, flush=True)
        comm, states, bs = _dist_states(kind)
        kw = dict(kw)
        kw.setdefault("max_coarse_size", 10)
        with _Env(env):
            amg = D.DistributedAMG(comm, states, dim=3, device=0, **kw)
        paths[name] = [o.top.level_paths(l) for o in amg._dev.ops for l in range(amg.k)]
        rng = np.random.default_rng(0)
        b = [torch.from_numpy(rng.standard_normal(s.n * bs) * np.repeat(s.free, bs)).cuda() for s in states]
        xs = [torch.full((s.n * bs,), float("nan"), dtype=torch.float64, device="cuda") for s in states]
        for rep in range(3):                           # direct launches, capture, replay
            amg.Mult(b, xs)
            torch.cuda.synchronize()
            if rep != 1:
                store(f"{name}|Mult {'direct' if rep == 0 else 'replay'}", np.concatenate([x.cpu().numpy() for x in xs]))
    return paths


def _multi(store):
    import numpy as np
    import torch
    from ngsamg_amd._lib import NgsAMGError
    from ngsamg_amd.device import DeviceAMGMatrix
    plans = {}
    for name, (make, *args), kw, env, need in MULTI_CASES:
        print(name, flush=True)
        H, free, bs = make(*args)
        with _Env(env):
            dev = DeviceAMGMatrix(H, device=0, **kw)
        if need and not dev.multi_plan(4, need)["fused"]:
            sys.exit(f"{name}: the handle keeps the column loop under fuse={need!r}: {dev.multi_plan(4, need)['note']}")
        fr = np.repeat(np.asarray(free) > 0, bs).astype(np.float64)
        n, nx = dev.sizes[0], dev.ext_sizes[0]
        rng = np.random.default_rng(11)
        B, X0, V = rng.standard_normal((7, n)) * fr, rng.standard_normal((7, n)) * fr, rng.standard_normal((7, nx))
        plans[name] = [dev.level_paths(l) for l in range(dev.n_levels)]
        for fuse in FUSE_WORDS:
            plans[name].append({"fuse": fuse, "plan": [dev.multi_plan(k, fuse) for k in range(1, 9)],
                                "levels": [dev.multi_level_plan(l, fuse) for l in range(dev.n_levels)]})
            for k, il, on_dev in MULTI_SHAPES:
                def lay(M):                              # the (k, rows) block in the layout and kind of this call
                    M = np.array(M[:k].T if il else M[:k], order="C")
                    return torch.from_numpy(M).cuda() if on_dev else M

                def call(tag, f, outputs):               # outputs: indices of the results among the values f returns
                    try:
                        got = f()
                        torch.cuda.synchronize()
                        got = np.concatenate([np.asarray(got[i].cpu() if on_dev else got[i]).ravel() for i in outputs])
                    except NgsAMGError as e:               # a refusal is a result too: the text must stay
                        got = np.frombuffer(str(e).encode(), dtype=np.uint8)
                    store(f"{name}|fuse={fuse} k={k} il={il} dev={on_dev}|{tag}", got)

                nan = np.full((7, n), np.nan)
                for rep, graph in enumerate((True, True, False)):        # capture, replay, direct launches
                    call(f"MultMulti graph={graph} rep={rep}", lambda: (dev.MultMulti(lay(B), lay(nan), interleaved=il, graph=graph, fuse=fuse),), (0,))
                call("MatVecMulti", lambda: (dev.MatVecMulti(0, lay(V), lay(nan), interleaved=il, fuse=fuse),), (0,))
                for back in (False, True):
                    call(f"SmoothMulti back={back}", lambda: (dev.SmoothMulti(0, lay(X0), lay(B), back=back, interleaved=il, fuse=fuse),), (0,))
                call("DownMulti", lambda: dev.DownMulti(0, lay(B), interleaved=il, fuse=fuse), (0, 1))
                call("DownMulti x_given", lambda: dev.DownMulti(0, lay(B), lay(X0), x_given=True, interleaved=il, fuse=fuse), (1,))
    return plans


def child(out, families):
    import numpy as np
    os.makedirs(out, exist_ok=True)
    index = {}

    def store(name, v):
        assert name not in index, name
        index[name] = f"{len(index):04d}.npy"
        np.save(os.path.join(out, index[name]), v)

    paths = {}
    for family, run in (("single", _single), ("dist", _dist), ("multi", _multi)):
        if family in families:
            paths.update(run(store))
    with open(os.path.join(out, "index.json"), "w") as f:
        json.dump({"results": index, "level_paths": paths}, f, default=str)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--out", required=True)
    ap.add_argument("--report")
    ap.add_argument("--child")
    ap.add_argument("--parent-root")
    ap.add_argument("--cases", default="single,dist,multi", help="the families to run: single (CASES), dist (DIST_CASES), multi (MULTI_CASES)")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.cases.split(","))
    import numpy as np
    runs = (("tree", None), ("parent", os.path.abspath(a.parent_lib)))
    for tag, lib in runs:
        env = dict(os.environ)
        env.pop("NGSAMG_HIP_LIB", None)
        if lib:
            env["NGSAMG_HIP_LIB"] = lib
        tool = os.path.join(os.path.abspath(a.parent_root), "tools", "bits_vs_parent.py") if lib and a.parent_root else os.path.abspath(__file__)
        rc = subprocess.run([sys.executable, tool, "--child", os.path.abspath(os.path.join(a.out, tag)), "--out", os.path.abspath(a.out), "--cases", a.cases], env=env, timeout=900).returncode
        if rc != 0:
            sys.exit(f"the run with the {tag} library ended with status {rc}: nothing more is started")
    T, P = (json.load(open(os.path.join(a.out, tag, "index.json"))) for tag, _ in runs)
    lines, bad = [], 0
    for name in sorted(set(T["results"]) | set(P["results"])):
        same = name in T["results"] and name in P["results"]
        if same:
            x, y = (np.load(os.path.join(a.out, tag, I["results"][name])) for tag, I in (("tree", T), ("parent", P)))
            same = np.array_equal(x, y) and not np.isnan(x).any()
        bad += not same
        lines.append(("same  " if same else "DIFF  ") + name)
    nres, pbad = len(lines), 0
    for name in sorted(set(T["level_paths"]) | set(P["level_paths"])):
        same = T["level_paths"].get(name) == P["level_paths"].get(name)
        pbad += not same
        forms = " ".join(f"L{l}:{lp['gs_form']}/split={lp['gs_split']}" for l, lp in enumerate(T["level_paths"].get(name, [])) if lp.get("gs_form"))
        n_lev = sum("gs_form" in lp for lp in T["level_paths"].get(name, []))       # (a multi case: its plan dictionaries follow)
        need = {c[0]: c[4] for c in MULTI_CASES}.get(name)
        lines.append(("same  " if same else "DIFF  ") + f"{name}|level_paths of {n_lev} levels: {forms}" + (f" | fused under {need} in both builds" if need else ""))
    head = [f"results: {nres}   identical: {nres - bad}   different: {bad}",
            f"handles: {len(lines) - nres}   level_paths identical: {len(lines) - nres - pbad}   different: {pbad}",
            "verdict: " + ("IDENTICAL" if bad == 0 and pbad == 0 else "DIFFERENT"), "", "== cases (handle | call)"]
    text = "\n".join(head + lines) + "\n"
    print(text, end="")
    if a.report:
        with open(a.report, "w") as f:
            f.write(text)
    sys.exit(0 if bad == 0 and pbad == 0 else 1)


if __name__ == "__main__":
    main()
