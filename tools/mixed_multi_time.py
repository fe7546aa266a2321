"""The reduced-precision route of a high-order handle, timed:
forward_multi_dev against forward_multi_f32_dev at nrhs = 1 and 8 with their M2L / near
stage spans, the f32 operator's relative distance from the fp64 one per column, the time and
bytes of cache_f32, and an 8-source solve (restart 80, tol 1e-12) through
forward_solve_multi_dev and through forward_solve_multi_mixed_dev: wall time, steps, outer
counts, the split of f32 / fp64 passes and the solutions' distance.  mode_multi_time.py's
protocol: every leg 20 calls between two events after 3 warm-ups, repeated --repeats times
(median and (max - min) / median), then its stage spans from aniso_set_timing(1) over 5 more
calls.  The headline geometry by default.  One JSON line per result.
usage: mixed_multi_time.py --np 6|8 [--sz 1024] [--d 1] [--ks 5] [--ns 10] [--nrhs 1 8]
                           [--calls 20] [--repeats 3] [--solve 8] [--inner-tol 1e-4 1e-6]"""
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
ap.add_argument("--np", type=int, required=True, choices=[6, 8], help="Chebyshev order per dimension")
ap.add_argument("--max-level", type=int, default=20)
ap.add_argument("--nrhs", nargs="+", type=int, default=[1, 8])
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--solve", type=int, default=8, help="sources of the timed solves (0: none)")
ap.add_argument("--inner-tol", nargs="+", type=float, default=[1e-4, 1e-6])
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
    out = dict(leg=name, np=args.np, N=a.N, ms=round(ms, 4), runs=[round(r, 4) for r in runs],
               spread=round((max(runs) - min(runs)) / ms, 5), passes=a.mode_apply_calls().tolist(),
               stage_ms={k: round(float(v), 4) for k, v in st.items()}, **kw)
    print(json.dumps(out), flush=True)
    return out


a = aniso_amd.Aniso(args.sz, args.d, args.ks, args.g, args.ns, args.np, args.max_level)
xy = a.getNodes()
a.setCoeff(*main_coeffs(xy))
a.cache_block()
torch.cuda.synchronize()
t = time.perf_counter()
a.cache_f32()
torch.cuda.synchronize()
print(json.dumps(dict(leg="cache_f32", np=args.np, N=a.N, wall_ms=round(1e3 * (time.perf_counter() - t), 3),
                      f32_bytes=a.cache_f32_bytes(), shared_cache_bytes=a.cache_bytes()[1])), flush=True)
rng = np.random.default_rng(0)
nmax = max(args.nrhs)
X = torch.tensor(rng.uniform(-1, 1, (nmax, a.N)) + gaussian(xy), device="cuda")
O64, O32 = torch.zeros_like(X), torch.zeros_like(X)
for k in args.nrhs:
    r64 = leg(a, "forward_multi_dev", lambda: a.forward_multi_dev(X[:k], O64[:k]), nrhs=k)
    r32 = leg(a, "forward_multi_f32_dev", lambda: a.forward_multi_f32_dev(X[:k], O32[:k]), nrhs=k)
    # the operators' distance: (x - K x) - (x - K~ x) against K x
    Kx = X[:k] - O64[:k]
    err = (torch.linalg.norm(O32[:k] - O64[:k], dim=1) / torch.linalg.norm(Kx, dim=1)).cpu().tolist()
    print(json.dumps(dict(nrhs=k, f64_ms=r64["ms"], f32_ms=r32["ms"], f32_over_f64=round(r32["ms"] / r64["ms"], 4),
                          legs_spread=max(r64["spread"], r32["spread"]),
                          m2l_ms=[r64["stage_ms"].get("m2l"), r32["stage_ms"].get("m2l")],
                          near_ms=[r64["stage_ms"].get("near"), r32["stage_ms"].get("near")],
                          f32_vs_f64_per_column=err)), flush=True)
if args.solve > 0:  # main.cpp's rhs = K_0 q; GMRES(80) for several sources
    x, y = xy[:, 0], xy[:, 1]
    Q = torch.tensor(np.array([np.exp(-w * ((x - 0.5) ** 2 + (y - 0.5) ** 2))
                               for w in np.linspace(25.0, 100.0, args.solve)]), device="cuda")
    def solve_leg(name, run, **kw):
        """a warm-up (it grows the buffers), then --repeats timed runs: the median wall time"""
        walls, res = [], None
        for rep in range(args.repeats + 1):
            torch.cuda.synchronize()
            t = time.perf_counter()
            res = run()
            torch.cuda.synchronize()
            if rep > 0:
                walls.append(time.perf_counter() - t)
        wall = float(np.median(walls))
        return wall, res, dict(leg=name, np=args.np, N=a.N, sources=args.solve, wall_s=round(wall, 4),
                               walls=[round(w, 4) for w in walls], spread=round((max(walls) - min(walls)) / wall, 4), **kw)

    def run64():
        Xs = torch.zeros_like(Q)
        return (Xs,) + tuple(a.forward_solve_multi_dev(Q, Xs, restart=80, tol=1e-12, maxit=5))

    wall64, (ref, iters, relres, _), out = solve_leg("forward_solve_multi_dev", run64)
    print(json.dumps(dict(out, iters=iters.tolist(), relres=relres.tolist(),
                          operator_calls=len(a.forward_solve_calls()))), flush=True)
    for itol in args.inner_tol:
        def runmx():
            Xm = torch.zeros_like(Q)
            return (Xm,) + tuple(a.forward_solve_multi_mixed_dev(Q, Xm, restart=80, tol=1e-12, inner_tol=itol, maxit=5,
                                                                 max_outer=10))

        wall, (Xm, iters, outer, relres), out = solve_leg("forward_solve_multi_mixed_dev", runmx, inner_tol=itol)
        calls = a.forward_solve_mixed_calls()
        dist = (torch.linalg.norm(Xm - ref, dim=1) / torch.linalg.norm(ref, dim=1)).cpu().tolist()
        print(json.dumps(dict(out, over_fp64=round(wall / wall64, 4), iters=iters.tolist(), outer=outer.tolist(),
                              relres=relres.tolist(), f32_passes=int((calls[:, 0] == 32).sum()),
                              fp64_passes=int((calls[:, 0] == 64).sum()), x_vs_fp64_solve=dist)), flush=True)
