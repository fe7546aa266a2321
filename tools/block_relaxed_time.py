"""The relaxed-precision block solve, timed, per order in one process:
  pass:  block_op_dev(2) against block_op_f32_dev(2) -- the pass, its M2L span and its near
         span (aniso_set_timing), and the distance of the f32 operator from the fp64 one;
  solve: block_solve_dev against block_solve_relaxed_dev at relax in {0, 1e-7, 1e-6, 1e-5,
         1e-4, 1e-3, 1}, tol 1e-11 -- steps, f32 and fp64 passes, wall time, final relres;
  and the np = 4 block matvec of the same session beside them (--np4).
Every pass leg: 20 calls between two events after 3 warm-ups, repeated --repeats times (median
and spread), then the stage spans over 5 more calls.  Every solve: one warm-up run, then
--repeats timed runs.  The headline geometry by default.  One JSON line per leg.
usage: block_relaxed_time.py [--np 6 8] [--sz 1024] [--d 1] [--ks 5] [--ns 10] [--calls 20]
                             [--repeats 3] [--restart 60] [--tol 1e-11] [--maxit 20] [--np4]"""
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
ap.add_argument("--np", nargs="+", type=int, default=[6, 8], choices=[6, 8])
ap.add_argument("--max-level", type=int, default=20)
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--restart", type=int, default=60)
ap.add_argument("--tol", type=float, default=1e-11)
ap.add_argument("--maxit", type=int, default=20)
ap.add_argument("--relax", nargs="+", type=float, default=[0.0, 1e-7, 1e-6, 1e-5, 1e-4, 1e-3, 1.0])
ap.add_argument("--np4", action="store_true", help="the np = 4 block matvec of this session beside them")
ap.add_argument("--no-solve", action="store_true")
args = ap.parse_args()


def pass_leg(a, fn, **kw):
    """median ms per call of fn over the repeats, their spread, and the stage spans"""
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
    spans = []
    for _ in range(args.repeats):
        a.set_timing(1)
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        spans.append(a.stage_times())
        a.set_timing(0)
    med = {k: float(np.median([s[k] for s in spans])) for k in spans[0]}
    rec = dict(leg="pass", N=a.N, ms=round(ms, 4), runs=[round(r, 4) for r in runs],
               spread=round((max(runs) - min(runs)) / ms, 5), m2l_ms=round(med["m2l"], 4),
               m2l_runs=[round(float(s["m2l"]), 4) for s in spans], near_ms=round(med["near"], 4),
               near_runs=[round(float(s["near"]), 4) for s in spans],
               stage_ms={k: round(v, 4) for k, v in med.items()}, **kw)
    print(json.dumps(rec), flush=True)
    return rec


def solve_leg(a, rhs, relax, **kw):
    """relax None: block_solve_dev; else the relaxed entry.  One warm-up run (it grows the
    buffers and builds the mirrors), then the timed repeats."""
    walls, out = [], None
    for rep in range(args.repeats + 1):
        x = torch.zeros_like(rhs)
        torch.cuda.synchronize()
        t = time.perf_counter()
        if relax is None:
            out = a.block_solve_dev(rhs, x, restart=args.restart, tol=args.tol, maxit=args.maxit)
        else:
            out = a.block_solve_relaxed_dev(rhs, x, restart=args.restart, tol=args.tol, maxit=args.maxit, relax=relax)
        torch.cuda.synchronize()
        if rep:
            walls.append(time.perf_counter() - t)
    it, hist, rr = out
    calls = a.block_solve_relaxed_calls() if relax is not None else np.zeros(0, dtype=np.int32)
    wall = float(np.median(walls))
    rec = dict(leg="solve", N=a.N, entry="block_solve_dev" if relax is None else "block_solve_relaxed_dev",
               relax=relax, steps=int(it), relres=float(rr), f32_passes=int(np.sum(calls == 32)),
               fp64_passes=int(np.sum(calls == 64)), wall_s=round(wall, 4), walls=[round(w, 4) for w in walls],
               spread=round((max(walls) - min(walls)) / wall, 5), **kw)
    print(json.dumps(rec), flush=True)
    return rec, x


def handle(np_):
    a = aniso_amd.Aniso(args.sz, args.d, args.ks, args.g, args.ns, np_, args.max_level)
    xy = a.getNodes()
    a.setCoeff(*main_coeffs(xy))
    a.cache_block()
    return a, xy


if args.np4:
    a, xy = handle(4)
    U = torch.tensor(np.random.default_rng(0).uniform(-1, 1, (a.ks, a.N)) + gaussian(xy), device="cuda")
    O = torch.zeros_like(U)
    pass_leg(a, lambda: a.block_op_dev(2, U, O), np=4, entry="block_op_dev")
    a.close()
    del a, U, O
    torch.cuda.empty_cache()

for np_ in args.np:
    a, xy = handle(np_)
    U = torch.tensor(np.random.default_rng(0).uniform(-1, 1, (a.ks, a.N)) + gaussian(xy), device="cuda")
    O64, O32 = torch.zeros_like(U), torch.zeros_like(U)
    r64 = pass_leg(a, lambda: a.block_op_dev(2, U, O64), np=np_, entry="block_op_dev")
    r32 = pass_leg(a, lambda: a.block_op_f32_dev(2, U, O32), np=np_, entry="block_op_f32_dev")
    dist = {}
    for which in (0, 1, 2):
        a.block_op_dev(which, U, O64)
        a.block_op_f32_dev(which, U, O32)
        dist[which] = float(torch.linalg.norm(O32 - O64) / torch.linalg.norm(O64))
    print(json.dumps(dict(leg="pass ratio", np=np_, pass_ratio=round(r32["ms"] / r64["ms"], 4),
                          m2l_ratio=round(r32["m2l_ms"] / r64["m2l_ms"], 4),
                          near_ratio=round(r32["near_ms"] / r64["near_ms"], 4), f32_vs_fp64=dist,
                          cache_f32_bytes=a.cache_f32_bytes(), cache_bytes=a.cache_bytes())), flush=True)
    if not args.no_solve:
        F = torch.tensor(np.stack([gaussian(xy) * (0.5 ** b) for b in range(a.ks)]), device="cuda")
        rhs = torch.zeros_like(F)
        a.block_op_dev(0, F, rhs)
        base, x64 = solve_leg(a, rhs, None, np=np_)
        for relax in args.relax:
            rec, x = solve_leg(a, rhs, relax, np=np_)
            print(json.dumps(dict(leg="solve ratio", np=np_, relax=relax, wall_ratio=round(rec["wall_s"] / base["wall_s"], 4),
                                  steps=rec["steps"], fp64_steps=base["steps"],
                                  solution_vs_fp64=float(torch.linalg.norm(x - x64) / torch.linalg.norm(x64)))),
                  flush=True)
    a.close()
    del a, U, O64, O32
    torch.cuda.empty_cache()
