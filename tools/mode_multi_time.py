"""One mode on several vectors on the mode-shared caches, timed: the
existing single-vector route mapping_dev (one 8-row pass of the block operator's offset
form) against mapping_multi_dev (the mode kernels of mode_apply.hip) at nrhs = 1 and 8,
with block_op_dev(2) as the session's yardstick.  Every leg: 20 calls between two events
after 3 warm-ups, repeated --repeats times (median and spread), then its stage spans from
aniso_set_timing(1) over 5 more calls.  The headline geometry by default.  One JSON line
per leg.  --np 4: the handle is lean (aniso_cache_block only); a second leg times the
resident route on a handle with aniso_cache(mode), and --solve k a k-source
forward_solve_multi_dev (restart 80, tol 1e-12) on the lean handle.
usage: mode_multi_time.py --np 6 [--sz 1024] [--d 1] [--ks 5] [--ns 10] [--modes 0 8]
                          [--nrhs 1 8] [--calls 20] [--repeats 3] [--solve 4]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import aniso_amd  # noqa: E402
from bench import gaussian, main_coeffs  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sz", type=int, default=1024)
ap.add_argument("--d", type=int, default=1)
ap.add_argument("--ks", type=int, default=5)
ap.add_argument("--ns", type=int, default=10)
ap.add_argument("--g", type=float, default=0.8)
ap.add_argument("--np", type=int, default=6, choices=[4, 6, 8], help="Chebyshev order per dimension")
ap.add_argument("--max-level", type=int, default=20)
ap.add_argument("--modes", nargs="+", type=int, default=None, help="default: 0 and 2ks - 2")
ap.add_argument("--nrhs", nargs="+", type=int, default=[1, 8])
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--solve", type=int, default=0, help="np 4: also time a forward solve of this many sources")
args = ap.parse_args()


def leg(a, name, fn, **kw):
    """median ms per call of fn over the repeats, their spread and the stage spans."""
    for _ in range(3):
        fn()
    runs = []
    for _ in range(args.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(args.calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        runs.append(e0.elapsed_time(e1) / args.calls)
    ms = float(np.median(runs))
    a.set_timing(1)
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    st = a.stage_times()
    a.set_timing(0)
    if kw.pop("passes", False):  # the compiled column count of every pass of the last call
        kw["passes"] = a.mode_apply_calls().tolist()
    print(json.dumps(dict(leg=name, np=args.np, N=a.N, ms=round(ms, 4), runs=[round(r, 4) for r in runs],
                          spread=round((max(runs) - min(runs)) / ms, 5),
                          stage_ms={k: round(float(v), 4) for k, v in st.items()}, **kw)), flush=True)
    return ms


a = aniso_amd.Aniso(args.sz, args.d, args.ks, args.g, args.ns, args.np, args.max_level)
xy = a.getNodes()
a.setCoeff(*main_coeffs(xy))
a.cache_block()
rng = np.random.default_rng(0)
nmax = max(args.nrhs)
X = torch.tensor(rng.uniform(-1, 1, (nmax, a.N)) + gaussian(xy), device="cuda")
Out = torch.zeros_like(X)
U = torch.tensor(rng.uniform(-1, 1, (args.ks, a.N)), device="cuda")
Y = torch.zeros_like(U)
block = leg(a, "block_op_dev(2)", lambda: a.block_op_dev(2, U, Y))
for m in (args.modes if args.modes is not None else [0, 2 * args.ks - 2]):
    q, o = X[0].contiguous(), torch.zeros(a.N, dtype=torch.float64, device="cuda")
    old = leg(a, "mapping_dev", lambda: a.mapping_dev(q, m, o), mode=m)
    ref = o.clone()
    one = None
    for k in args.nrhs:
        ms = leg(a, "mapping_multi_dev", lambda: a.mapping_multi_dev(X[:k], m, Out[:k]), mode=m, nrhs=k,
                 passes=True)
        if k == 1:
            one = ms
        err = float(torch.linalg.norm(Out[0] - ref) / torch.linalg.norm(ref))
        print(json.dumps(dict(mode=m, nrhs=k, ms=round(ms, 4), per_column_ms=round(ms / k, 4),
                              over_mapping_dev=round(ms / old, 4), over_one_column=round(ms / one, 4) if one else None,
                              over_block_op=round(ms / block, 4), column0_vs_mapping_dev=err)), flush=True)
if args.np == 4:
    if args.solve > 0:  # main.cpp's rhs = K_0 q; GMRES(80) for several sources, lean
        x, y = xy[:, 0], xy[:, 1]
        Q = torch.tensor(np.array([np.exp(-w * ((x - 0.5) ** 2 + (y - 0.5) ** 2))
                                   for w in np.linspace(25.0, 100.0, args.solve)]), device="cuda")
        for rep in range(2):  # the first run grows the buffers
            Xs = torch.zeros_like(Q)
            torch.cuda.synchronize()
            t = time.perf_counter()
            iters, relres, _ = a.forward_solve_multi_dev(Q, Xs, restart=80, tol=1e-12, maxit=5)
            torch.cuda.synchronize()
            wall = time.perf_counter() - t
            print(json.dumps(dict(leg="forward_solve_multi_dev", lean=True, sources=args.solve, run=rep,
                                  wall_s=round(wall, 4), iters=iters.tolist(), relres=relres.tolist(),
                                  operator_calls=len(a.forward_solve_calls()),
                                  last_passes=a.mode_apply_calls().tolist())), flush=True)
    # the resident route: the mode's own operators (aniso_cache(mode)), applyBlock's batched branch
    for m in (args.modes if args.modes is not None else [0]):
        a.cache(m)
        per_mode = a.cache_bytes()[0]
        for k in args.nrhs:
            leg(a, "mapping_multi_dev resident", lambda: a.mapping_multi_dev(X[:k], m, Out[:k]), mode=m, nrhs=k,
                passes=True, per_mode_cache_bytes=per_mode)
