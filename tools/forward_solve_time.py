"""The multi-source forward solve, timed: 8 Gaussian sources at different
centres through forward_solve_multi_dev (restart 80, tol 1e-12) on the headline geometry
with main.cpp's coefficients.  Prints the steps per column, the operator calls with the
column count of each (the compaction), the solve's time, and -- in the same process -- the
time of forward_multi_dev at each of those column counts: the yardstick.  The figure is
    solve time / sum over the operator calls of the yardstick at the call's column count;
what exceeds 1 is the Krylov layer (sweeps, small kernels, the host's wait per step).  Then
one 8-source call against eight 1-source calls.  One JSON line per result.  Manual: no test
and no benchmark runs it.
usage: forward_solve_time.py --np 6 [--sz 1024] [--d 1] [--ks 5] [--ns 10] [--restart 80]"""
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
ap.add_argument("--np", type=int, default=6, choices=[4, 6, 8], help="Chebyshev order per dimension")
ap.add_argument("--max-level", type=int, default=20)
ap.add_argument("--restart", type=int, default=80)
ap.add_argument("--tol", type=float, default=1e-12)
ap.add_argument("--maxit", type=int, default=5)
ap.add_argument("--calls", type=int, default=10, help="yardstick calls per column count")
args = ap.parse_args()

a = aniso_amd.Aniso(args.sz, args.d, args.ks, args.g, args.ns, args.np, args.max_level)
xy = a.getNodes()
a.setCoeff(*main_coeffs(xy))
a.cache_block()
N = a.N
centres = [(0.5, 0.5), (0.25, 0.25), (0.75, 0.25), (0.25, 0.75), (0.75, 0.75), (0.5, 0.2), (0.2, 0.5), (0.8, 0.6)]
Q = torch.tensor(np.array([np.exp(-25.0 * ((xy[:, 0] - cx) ** 2 + (xy[:, 1] - cy) ** 2)) for cx, cy in centres]),
                 device="cuda")


def solve(rows):
    """(seconds, iters, relres, operator calls) of one call on Q[rows] from a zero guess."""
    X = torch.zeros(len(rows), N, dtype=torch.float64, device="cuda")
    q = Q[rows].contiguous()
    torch.cuda.synchronize()
    t = time.perf_counter()
    iters, relres, _ = a.forward_solve_multi_dev(q, X, restart=args.restart, tol=args.tol, maxit=args.maxit)
    torch.cuda.synchronize()
    return time.perf_counter() - t, iters, relres, a.forward_solve_calls().tolist()


solve(list(range(8)))  # warm-up: work buffers, kernels loaded
sec8, iters, relres, calls = solve(list(range(8)))
print(json.dumps(dict(np=args.np, N=N, restart=args.restart, tol=args.tol, steps=iters.tolist(),
                      relres=[float(f"{r:.3e}") for r in relres])), flush=True)
print(json.dumps(dict(operator_calls=len(calls), columns_per_call=calls)), flush=True)

# the yardstick: forward_multi_dev at every column count an operator call had
yard = {}
Out = torch.zeros(8, N, dtype=torch.float64, device="cuda")
for k in sorted(set(calls)):
    for _ in range(3):
        a.forward_multi_dev(Q[:k], Out[:k])
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(args.calls):
        a.forward_multi_dev(Q[:k], Out[:k])
    e1.record()
    torch.cuda.synchronize()
    yard[k] = e0.elapsed_time(e1) / args.calls
print(json.dumps(dict(forward_multi_dev_ms={k: round(v, 4) for k, v in yard.items()})), flush=True)
ops = sum(yard[k] for k in calls)  # (the right-hand sides' mapping pass is not among the calls)
print(json.dumps(dict(solve_ms=round(1e3 * sec8, 3), operator_calls_ms=round(ops, 3),
                      solve_over_operator_calls=round(1e3 * sec8 / ops, 4))), flush=True)

one = [solve([k]) for k in range(8)]
sec1 = sum(o[0] for o in one)
print(json.dumps(dict(eight_sources_one_call_ms=round(1e3 * sec8, 3), eight_calls_of_one_source_ms=round(1e3 * sec1, 3),
                      steps_alone=[int(o[1][0]) for o in one], ratio=round(sec1 / sec8, 3))), flush=True)
