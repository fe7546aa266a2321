"""The relaxed-precision multi-source operator and lockstep solves, timed,
one order per process, tools/block_relaxed_time.py's protocol:
  block solve:   4 Gaussian charges (tools/block_multi_time.py's), restart 80, tol 1e-11:
                 block_solve_multi_dev against block_solve_multi_relaxed_dev at relax in
                 {0, 1e-7, 1e-6, 1e-5, 1e-4, 1} -- steps, f32 / fp64 calls, wall time, relres,
                 distance of the solutions;
  forward solve: 8 sources (16 with --wide on top), restart 80, tol 1e-12:
                 forward_solve_multi_dev against forward_solve_multi_relaxed_dev at relax in
                 {0, 1e-8, 1e-7, 1e-6, 1e-5, 1}, and forward_solve_multi_mixed_dev beside them;
  pass:          block_op_multi_dev(2) against block_op_multi_f32_dev(2) on 4, 2 and 1 sources --
                 the pass, its M2L span and its near span (aniso_set_timing).
The solves run BEFORE the legs (a multi-source solve is dearer after the
legs have recorded timing events).  Every solve: one warm-up run, then --repeats timed runs,
median and spread; the fp64 entry is timed before and again after the relaxed runs.  Every
pass leg: 20 calls between two events after 3 warm-ups, --repeats times.  The headline
geometry by default.  One JSON line per leg.
usage: multi_relaxed_time.py --np 6|8 [--sz 1024] [--d 1] [--ks 5] [--ns 10] [--calls 20]
                             [--repeats 5] [--wide] [--no-solve] [--no-forward] [--no-pass]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import aniso_amd  # noqa: E402
from bench import main_coeffs  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sz", type=int, default=1024)
ap.add_argument("--d", type=int, default=1)
ap.add_argument("--ks", type=int, default=5)
ap.add_argument("--ns", type=int, default=10)
ap.add_argument("--g", type=float, default=0.8)
ap.add_argument("--np", type=int, default=6, choices=[6, 8])
ap.add_argument("--max-level", type=int, default=20)
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--restart", type=int, default=80)
ap.add_argument("--maxit", type=int, default=5)
ap.add_argument("--wide", action="store_true", help="also 16 forward sources with aniso_set_wide on")
ap.add_argument("--no-solve", action="store_true")
ap.add_argument("--no-forward", action="store_true")
ap.add_argument("--no-pass", action="store_true")
args = ap.parse_args()

a = aniso_amd.Aniso(args.sz, args.d, args.ks, args.g, args.ns, args.np, args.max_level)
xy = a.getNodes()
a.setCoeff(*main_coeffs(xy))
a.cache_block()
N, ks = a.N, a.ks


def solve_leg(name, run, **kw):
    """A warm-up (it grows the buffers and builds the mirrors), then the timed repeats."""
    walls, res = [], None
    for rep in range(args.repeats + 1):
        torch.cuda.synchronize()
        t = time.perf_counter()
        res = run()
        torch.cuda.synchronize()
        if rep:
            walls.append(time.perf_counter() - t)
    wall = float(np.median(walls))
    return wall, res, dict(leg=name, np=args.np, N=N, wall_s=round(wall, 4), walls=[round(w, 4) for w in walls],
                           spread=round((max(walls) - min(walls)) / wall, 4), **kw)


def report(out, wall, wall64, X, ref, iters, relres, relaxed):
    calls = a.solve_multi_relaxed_calls() if relaxed else np.zeros((0, 2), dtype=np.int32)
    rows = X.reshape(len(iters), -1), ref.reshape(len(iters), -1)
    dist = (torch.linalg.norm(rows[0] - rows[1], dim=1) / torch.linalg.norm(rows[1], dim=1)).cpu().tolist()
    print(json.dumps(dict(out, over_fp64=round(wall / wall64, 4), steps=iters.tolist(),
                          relres=[float(f"{r:.3e}") for r in relres], f32_calls=int((calls[:, 0] == 32).sum()),
                          fp64_calls=int((calls[:, 0] == 64).sum()), x_vs_fp64_solve=[float(f"{d:.3e}") for d in dist])),
          flush=True)


if not args.no_solve:
    centres = [(0.5, 0.5), (0.25, 0.25), (0.75, 0.25), (0.25, 0.75)]  # block b scaled by 2^-b
    Q = torch.tensor(np.array([np.exp(-25.0 * ((xy[:, 0] - cx) ** 2 + (xy[:, 1] - cy) ** 2)) * 0.5 ** b
                               for cx, cy in centres for b in range(ks)]), device="cuda")
    tol = 1e-11

    def run64():
        Xs = torch.zeros_like(Q)
        return (Xs,) + tuple(a.block_solve_multi_dev(Q, Xs, restart=args.restart, tol=tol, maxit=args.maxit))

    wall64, (ref, iters, relres, _), out = solve_leg("block_solve_multi_dev", run64, sources=4)
    report(out, wall64, wall64, ref, ref, iters, relres, False)
    for relax in (0.0, 1e-7, 1e-6, 1e-5, 1e-4, 1.0):
        def runrx():
            Xs = torch.zeros_like(Q)
            return (Xs,) + tuple(a.block_solve_multi_relaxed_dev(Q, Xs, restart=args.restart, tol=tol, maxit=args.maxit,
                                                                 relax=relax))

        wall, (Xs, iters, relres, _), out = solve_leg("block_solve_multi_relaxed_dev", runrx, sources=4, relax=relax)
        report(out, wall, wall64, Xs, ref, iters, relres, True)
    # the yardstick once more, after the relaxed runs: the two fp64 figures bracket the session
    wall, (Xs, iters, relres, _), out = solve_leg("block_solve_multi_dev", run64, sources=4, again=True)
    report(out, wall, wall64, Xs, ref, iters, relres, False)
    del Q

if not args.no_forward:
    x, y = xy[:, 0], xy[:, 1]
    tol = 1e-12
    for wide, n in [(False, 8)] + ([(True, 16)] if args.wide else []):
        a.set_wide(wide)
        Q = torch.tensor(np.array([np.exp(-w * ((x - 0.5) ** 2 + (y - 0.5) ** 2)) for w in np.linspace(25.0, 100.0, n)]),
                         device="cuda")

        def run64():
            Xs = torch.zeros_like(Q)
            return (Xs,) + tuple(a.forward_solve_multi_dev(Q, Xs, restart=args.restart, tol=tol, maxit=args.maxit))

        wall64, (ref, iters, relres, _), out = solve_leg("forward_solve_multi_dev", run64, sources=n, wide=wide)
        report(out, wall64, wall64, ref, ref, iters, relres, False)
        for relax in (0.0, 1e-8, 1e-7, 1e-6, 1e-5, 1.0):
            def runrx():
                Xs = torch.zeros_like(Q)
                return (Xs,) + tuple(a.forward_solve_multi_relaxed_dev(Q, Xs, restart=args.restart, tol=tol,
                                                                       maxit=args.maxit, relax=relax))

            wall, (Xs, iters, relres, _), out = solve_leg("forward_solve_multi_relaxed_dev", runrx, sources=n, wide=wide,
                                                          relax=relax)
            report(out, wall, wall64, Xs, ref, iters, relres, True)

        def runmx():
            Xm = torch.zeros_like(Q)
            return (Xm,) + tuple(a.forward_solve_multi_mixed_dev(Q, Xm, restart=args.restart, tol=tol, inner_tol=1e-4,
                                                                 maxit=args.maxit, max_outer=10))

        wall, (Xm, iters, outer, relres), out = solve_leg("forward_solve_multi_mixed_dev", runmx, sources=n, wide=wide)
        report(out, wall, wall64, Xm, ref, iters, relres, False)
        wall, (Xs, iters, relres, _), out = solve_leg("forward_solve_multi_dev", run64, sources=n, wide=wide, again=True)
        report(out, wall, wall64, Xs, ref, iters, relres, False)
        del Q
    a.set_wide(False)


def pass_leg(name, fn, **kw):
    """median ms per call over the repeats, their spread, and the stage spans"""
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
    rec = dict(leg=name, np=args.np, N=N, ms=round(ms, 4), runs=[round(r, 4) for r in runs], spread_ms=round(max(runs) - min(runs), 4),
               m2l_ms=round(float(st["m2l"]), 4), near_ms=round(float(st["near"]), 4), **kw)
    print(json.dumps(rec), flush=True)
    return rec


if not args.no_pass:
    X = torch.tensor(np.random.default_rng(0).uniform(-1, 1, (4 * ks, N)), device="cuda")
    O64, O32 = torch.zeros_like(X), torch.zeros_like(X)
    for n in (4, 2, 1):
        r64 = pass_leg("block_op_multi_dev", lambda: a.block_op_multi_dev(2, X[:n * ks], O64[:n * ks]), sources=n)
        r32 = pass_leg("block_op_multi_f32_dev", lambda: a.block_op_multi_f32_dev(2, X[:n * ks], O32[:n * ks]), sources=n)
        dist = float(torch.linalg.norm(O32[:n * ks] - O64[:n * ks]) / torch.linalg.norm(O64[:n * ks]))
        print(json.dumps(dict(leg="pass ratio", np=args.np, sources=n, f32_over_fp64=round(r32["ms"] / r64["ms"], 4),
                              saved_ms=round(r64["ms"] - r32["ms"], 4), spread_ms=max(r64["spread_ms"], r32["spread_ms"]),
                              m2l_ratio=round(r32["m2l_ms"] / r64["m2l_ms"], 4),
                              near_ratio=round(r32["near_ms"] / r64["near_ms"], 4), f32_vs_fp64=dist)), flush=True)
a.close()
