"""The wide setting of a high-order handle, timed: forward_multi_dev passes of
9, 12 and 16 columns and a 16-source forward solve with the setting off and on, in one process
on one handle, in three residency states of mode 0: nothing resident (the wide mode M2L
k_ho_m2l_mode_wide against two launches of k_ho_m2l_mode), the M2L blocks of cache_mode(0), and
the near blocks of cache_mode_near(0) as well.  The yardstick is the same handle with the
setting off.  A pass: 3 warm-ups, then --calls calls between two events, --repeats times, the
two settings taking turns (median and spread each), then its stage spans from
aniso_set_timing(1) over 5 more calls, summed over the call's passes.  The solve: Gaussian
sources exp(-w |x - c|^2), w = 25 .. 100, restart 80, tol 1e-12; whole-call wall time after one
warm-up solve, median of --repeats, the two settings taking turns.  The headline geometry by
default.  One JSON line per leg.
usage: wide_time.py --np 6 [--sz 1024] [--d 1] [--ks 5] [--ns 10] [--nrhs 9 12 16] [--calls 20]
                    [--repeats 3] [--solve 16] [--states nothing m2l both]"""
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
ap.add_argument("--np", type=int, default=6, choices=[6, 8], help="Chebyshev order per dimension")
ap.add_argument("--max-level", type=int, default=20)
ap.add_argument("--nrhs", nargs="+", type=int, default=[9, 12, 16])
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--solve", type=int, default=16, help="sources of the forward solve (0: none)")
ap.add_argument("--states", nargs="+", default=["nothing", "m2l", "both"], choices=["nothing", "m2l", "both"])
args = ap.parse_args()

SETTINGS = (("off", False), ("on", True))


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(args.calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / args.calls


def passes(a, state, X, Out):
    """The pass of every column count, the two settings taking turns within a repeat."""
    for k in args.nrhs:
        fn = lambda: a.forward_multi_dev(X[:k], Out[:k])  # noqa: E731
        runs = {name: [] for name, _ in SETTINGS}
        for name, on in SETTINGS:
            a.set_wide(on)
            for _ in range(3):
                fn()
        for _ in range(args.repeats):
            for name, on in SETTINGS:
                a.set_wide(on)
                runs[name].append(timed(fn))
        rec = dict(leg="forward_multi_dev", np=args.np, N=a.N, state=state, nrhs=k)
        outs = {}
        for name, on in SETTINGS:
            a.set_wide(on)
            a.set_timing(1)
            for _ in range(5):
                fn()
            torch.cuda.synchronize()
            st = a.stage_times()
            a.set_timing(0)
            chunks = a.mode_apply_calls().tolist()
            near = a.mode_near_calls().tolist()
            ms = float(np.median(runs[name]))
            rec[name] = dict(ms=round(ms, 4), runs=[round(r, 4) for r in runs[name]],
                             spread=round((max(runs[name]) - min(runs[name])) / ms, 5), chunks=chunks, near=near,
                             # (stage spans are means per pass: summed over the call's passes)
                             m2l_ms=round(float(st["m2l"]) * len(chunks), 4), near_ms=round(float(st["near"]) * len(chunks), 4))
            outs[name] = Out[:k].clone()
        rec["ratio"] = round(rec["on"]["ms"] / rec["off"]["ms"], 4)
        rec["m2l_ratio"] = round(rec["on"]["m2l_ms"] / rec["off"]["m2l_ms"], 4) if rec["off"]["m2l_ms"] > 0 else None
        rec["bitwise_equal"] = bool(torch.equal(outs["on"], outs["off"]))
        rec["worst_column_on_vs_off"] = float((torch.linalg.norm(outs["on"] - outs["off"], dim=1) /
                                               torch.linalg.norm(outs["off"], dim=1)).max())
        print(json.dumps(rec), flush=True)


def solves(a, state, Q):
    def one():
        Xs = torch.zeros_like(Q)
        torch.cuda.synchronize()
        t = time.perf_counter()
        iters, relres, _ = a.forward_solve_multi_dev(Q, Xs, restart=80, tol=1e-12, maxit=5)
        torch.cuda.synchronize()
        return time.perf_counter() - t, iters, relres, Xs

    walls = {name: [] for name, _ in SETTINGS}
    last = {}
    for name, on in SETTINGS:  # the warm-up solve grows the buffers
        a.set_wide(on)
        one()
    for _ in range(args.repeats):
        for name, on in SETTINGS:
            a.set_wide(on)
            w, iters, relres, Xs = one()
            walls[name].append(w)
            calls = a.forward_solve_calls().tolist()
            last[name] = dict(iters=iters.tolist(), worst_relres=float(relres.max()), operator_calls=len(calls),
                              rows=int(sum(calls)), calls_by_rows={str(r): calls.count(r) for r in sorted(set(calls))}, x=Xs)
    rec = dict(leg="forward_solve_multi_dev", np=args.np, N=a.N, state=state, sources=int(Q.shape[0]))
    xs = {}
    for name, _ in SETTINGS:
        xs[name] = last[name].pop("x")
        s = float(np.median(walls[name]))
        rec[name] = dict(wall_s=round(s, 4), runs=[round(w, 4) for w in walls[name]],
                         spread=round((max(walls[name]) - min(walls[name])) / s, 5), **last[name])
    rec["ratio"] = round(rec["on"]["wall_s"] / rec["off"]["wall_s"], 4)
    rec["bitwise_equal"] = bool(torch.equal(xs["on"], xs["off"]))
    rec["worst_column_on_vs_off"] = float((torch.linalg.norm(xs["on"] - xs["off"], dim=1) /
                                           torch.linalg.norm(xs["off"], dim=1)).max())
    print(json.dumps(rec), flush=True)


a = aniso_amd.Aniso(args.sz, args.d, args.ks, args.g, args.ns, args.np, args.max_level)
xy = a.getNodes()
a.setCoeff(*main_coeffs(xy))
a.cache_block()
rng = np.random.default_rng(0)
nmax = max(args.nrhs)
X = torch.tensor(rng.uniform(-1, 1, (nmax, a.N)) + gaussian(xy), device="cuda")
Out = torch.zeros_like(X)
Q = None
if args.solve > 0:  # main.cpp's rhs = K_0 q
    x, y = xy[:, 0], xy[:, 1]
    Q = torch.tensor(np.array([np.exp(-w * ((x - 0.5) ** 2 + (y - 0.5) ** 2))
                               for w in np.linspace(25.0, 100.0, args.solve)]), device="cuda")

for state in args.states:
    a.cache_mode_free()
    a.cache_mode_near_free()
    if state in ("m2l", "both"):
        a.cache_mode(0)
    if state == "both":
        a.cache_mode_near(0)
    print(json.dumps(dict(leg="state", np=args.np, state=state, cache_mode_bytes=a.cache_mode_bytes(),
                          cache_mode_near_bytes=a.cache_mode_near_bytes(), cache_bytes=a.cache_bytes())), flush=True)
    passes(a, state, X, Out)
    if Q is not None:
        solves(a, state, Q)
a.set_wide(False)
a.cache_mode_free()
a.cache_mode_near_free()
