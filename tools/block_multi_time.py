"""The block operator and its solve for several sources on a high-order handle, timed
(DESIGN.md §3.18.3): block_op_multi_dev(2, nsrc) at nsrc = 1, 2, 4 and 8 against
block_op_dev(2) of the same handle in the same process -- the yardstick, the existing entry.
Every leg: 20 calls between two events after 3 warm-ups, repeated 3 times (the spread), then
its M2L and near-field spans from aniso_set_timing(1) over 5 more calls.  Before the legs, one
solve: 4 Gaussian charges through block_solve_multi_dev (restart 80, tol 1e-11, zero guess),
compared with the sum of block_op_multi_dev's time over its operator calls at each call's
source count, and with four 1-source block_solve_dev calls.  The headline geometry by default.  One JSON line per
result.  Manual: no test and no benchmark runs it.
usage: block_multi_time.py --np 6 [--sz 1024] [--d 1] [--ks 5] [--ns 10] [--nsrc 1 2 4 8]
                           [--calls 20] [--repeats 3] [--restart 80] [--no-solve]"""
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
ap.add_argument("--nsrc", nargs="+", type=int, default=[1, 2, 4, 8])
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--restart", type=int, default=80)
ap.add_argument("--tol", type=float, default=1e-11)
ap.add_argument("--maxit", type=int, default=5)
ap.add_argument("--no-solve", action="store_true")
args = ap.parse_args()


def timed(fn, calls):
    """ms per call: `calls` calls between two events."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def leg(a, name, fn, **kw):
    """The repeats of a leg (ms per call each) and its stage spans; returns the median."""
    for _ in range(3):
        fn()
    ms = [timed(fn, args.calls) for _ in range(args.repeats)]
    a.set_timing(1)
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    st = a.stage_times()
    a.set_timing(0)
    print(json.dumps(dict(leg=name, np=args.np, N=a.N, ms=[round(m, 4) for m in ms],
                          m2l_ms=round(float(st["m2l"]), 4), near_ms=round(float(st["near"]), 4),
                          total_ms=round(float(st["total"]), 4), **kw)), flush=True)
    return float(np.median(ms)), max(ms) - min(ms)


a = aniso_amd.Aniso(args.sz, args.d, args.ks, args.g, args.ns, args.np, args.max_level)
xy = a.getNodes()
a.setCoeff(*main_coeffs(xy))
a.cache_block()
N, ks = a.N, a.ks
rng = np.random.default_rng(0)
nmax = max(args.nsrc)
X = torch.tensor(rng.uniform(-1, 1, (nmax * ks, N)), device="cuda")
Out = torch.zeros_like(X)
Y = torch.zeros(ks, N, dtype=torch.float64, device="cuda")
# 4 Gaussian charges, block b scaled by 2^-b
centres = [(0.5, 0.5), (0.25, 0.25), (0.75, 0.25), (0.25, 0.75)]
Q = torch.tensor(np.array([np.exp(-25.0 * ((xy[:, 0] - cx) ** 2 + (xy[:, 1] - cy) ** 2)) * 0.5 ** b
                           for cx, cy in centres for b in range(ks)]), device="cuda")


def solve4():
    """(seconds, iters, relres, operator calls) of one 4-source solve from a zero guess."""
    Xs = torch.zeros_like(Q)
    torch.cuda.synchronize()
    t = time.perf_counter()
    iters, relres, _ = a.block_solve_multi_dev(Q, Xs, restart=args.restart, tol=args.tol, maxit=args.maxit)
    torch.cuda.synchronize()
    return time.perf_counter() - t, iters, relres, a.forward_solve_calls().tolist()


def solve1(b):
    """(seconds, steps) of one block_solve_dev on the right-hand side b from a zero guess."""
    x = torch.zeros_like(b)
    torch.cuda.synchronize()
    t = time.perf_counter()
    it, _, _ = a.block_solve_dev(b, x, restart=args.restart, tol=args.tol, maxit=args.maxit)
    torch.cuda.synchronize()
    return time.perf_counter() - t, int(it)


# The solves run BEFORE the legs.  Measured at np = 6: the same 4-source solve (39 operator
# calls) takes 0.69 s here and 1.31 s after the legs, which record timing events (torch's and
# aniso_set_timing's); four block_solve_dev calls take 1.23 s either way.  The multi-source
# solve issues about a hundred launches per operator call and waits for the host once per
# step without a look-ahead call, so it is the one that shows a dearer launch.
if not args.no_solve:
    solve4()  # warm-up: work buffers, kernels loaded
    sec4, iters, relres, calls = solve4()
    print(json.dumps(dict(np=args.np, N=N, restart=args.restart, tol=args.tol, steps=iters.tolist(),
                          relres=[float(f"{r:.3e}") for r in relres], operator_calls=len(calls),
                          sources_per_call=calls)), flush=True)
    B = torch.zeros_like(Q)
    a.block_op_multi_dev(0, Q, B)  # b = forward(q)
    rhs = [B[s * ks:(s + 1) * ks].contiguous() for s in range(4)]
    solve1(rhs[0])  # warm-up
    alone = [solve1(b) for b in rhs]
    sec1 = sum(t for t, _ in alone)

yard, yspread = leg(a, "block_op_dev(2)", lambda: a.block_op_dev(2, X[:ks], Y))
ref = Y.clone()
multi = {}
for n in args.nsrc:
    ms, spread = leg(a, "block_op_multi_dev(2)", lambda: a.block_op_multi_dev(2, X[:n * ks], Out[:n * ks]), nsrc=n)
    multi[n] = ms
    err = float(torch.linalg.norm(Out[:ks] - ref) / torch.linalg.norm(ref))
    print(json.dumps(dict(nsrc=n, ms=round(ms, 4), spread_ms=round(spread, 4), per_source_ms=round(ms / n, 4),
                          over_n_yardsticks=round(ms / (n * yard), 4), yardstick_ms=round(yard, 4),
                          yardstick_spread_ms=round(yspread, 4), source0_vs_block_op_dev=err)), flush=True)
if args.no_solve:
    sys.exit(0)

# the solve against its operator calls at each call's source count, and against four solves alone
for k in sorted(set(calls)):
    if k not in multi:
        fn = lambda: a.block_op_multi_dev(2, X[:k * ks], Out[:k * ks])  # noqa: E731
        for _ in range(3):
            fn()
        multi[k] = timed(fn, args.calls)
ops = sum(multi[k] for k in calls)
print(json.dumps(dict(solve_ms=round(1e3 * sec4, 3), operator_calls_ms=round(ops, 3),
                      solve_over_operator_calls=round(1e3 * sec4 / ops, 4),
                      block_op_multi_dev_ms={k: round(multi[k], 4) for k in sorted(set(calls))})), flush=True)
print(json.dumps(dict(four_sources_one_call_ms=round(1e3 * sec4, 3), four_block_solve_dev_calls_ms=round(1e3 * sec1, 3),
                      steps_alone=[it for _, it in alone], ratio=round(sec1 / sec4, 3))), flush=True)
