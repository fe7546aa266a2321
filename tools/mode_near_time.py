"""The resident near field of a high-order handle, timed: a mode's pass and
its near span at 1, 8 and 16 columns in the four states {nothing, M2L blocks, near blocks, M2L +
near blocks} resident, in one process on one handle; the build of the near blocks and their
bytes against the directed near E blocks; the near launch's stored bytes over its span; the
worst column against the state with nothing resident; and an 8-source forward solve on the M2L
blocks with and without the near blocks.  Every leg: 20 calls between two events after 3
warm-ups, repeated --repeats times (median and spread), then its stage spans from
aniso_set_timing(1) over 5 more calls.  The headline geometry by default.  One JSON line per leg.
usage: mode_near_time.py --np 6 [--sz 1024] [--d 1] [--ks 5] [--ns 10] [--modes 0 8]
                         [--nrhs 1 8 16] [--calls 20] [--repeats 3] [--solve 8]"""
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
ap.add_argument("--modes", nargs="+", type=int, default=[0, 8])
ap.add_argument("--nrhs", nargs="+", type=int, default=[1, 8, 16])
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--solve", type=int, default=8, help="sources of the forward solve (0: none)")
args = ap.parse_args()

ACHIEVABLE_TBS = 6.3  # the stream rate HBM sustains
STATES = ["nothing", "M2L", "near", "M2L + near"]


def leg(a, fn, **kw):
    """median ms per call of fn over the repeats, their spread and the stage spans; near_ms: the
    near spans of one call (a stage span is a mean per pass: summed over the call's passes)."""
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
    near_runs = []
    for _ in range(args.repeats):
        a.set_timing(1)
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        st = a.stage_times()
        a.set_timing(0)
        near_runs.append(float(st["near"]) * len(a.mode_apply_calls()))
    near = float(np.median(near_runs))
    nc = a.mode_near_calls()
    rec = dict(leg="mapping_multi_dev", np=args.np, N=a.N, ms=round(ms, 4), runs=[round(r, 4) for r in runs],
               spread=round((max(runs) - min(runs)) / ms, 5), passes=a.mode_apply_calls().tolist(),
               near_launches=nc[:, 0].tolist(), near_resident=nc[:, 1].tolist(), near_ms=round(near, 4),
               near_runs=[round(r, 4) for r in near_runs], near_spread=round((max(near_runs) - min(near_runs)) / near, 5),
               stage_ms={k: round(float(v), 4) for k, v in st.items()}, **kw)
    print(json.dumps(rec), flush=True)
    return rec


def solve(a, Q, label):
    for rep in range(2):  # the first run grows the buffers
        Xs = torch.zeros_like(Q)
        torch.cuda.synchronize()
        t = time.perf_counter()
        iters, relres, _ = a.forward_solve_multi_dev(Q, Xs, restart=80, tol=1e-12, maxit=5)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t
        nc = a.mode_near_calls()
        print(json.dumps(dict(leg="forward_solve_multi_dev", route=label, sources=int(Q.shape[0]), run=rep,
                              wall_s=round(wall, 4), iters=iters.tolist(), relres=relres.tolist(),
                              operator_calls=len(a.forward_solve_calls()), last_passes=a.mode_apply_calls().tolist(),
                              last_near=nc.tolist())), flush=True)


def state(a, m, name):
    a.cache_mode_free()
    a.cache_mode_near_free()
    if "M2L" in name:
        a.cache_mode(m)
    if "near" in name:
        a.cache_mode_near(m)


a = aniso_amd.Aniso(args.sz, args.d, args.ks, args.g, args.ns, args.np, args.max_level)
xy = a.getNodes()
a.setCoeff(*main_coeffs(xy))
a.cache_block()
rng = np.random.default_rng(0)
nmax = max(args.nrhs)
X = torch.tensor(rng.uniform(-1, 1, (nmax, a.N)) + gaussian(xy), device="cuda")
Out = torch.zeros_like(X)
near_e_bytes = a.stats()["stored_near"] * 8  # (the directed near E blocks without their row padding)

for m in args.modes:
    torch.cuda.synchronize()
    t = time.perf_counter()
    a.cache_mode_near(m)
    build_s = time.perf_counter() - t
    nbytes = a.cache_mode_near_bytes()
    print(json.dumps(dict(leg="cache_mode_near", np=args.np, mode=m, wall_s=round(build_s, 4), bytes=nbytes,
                          near_e_bytes=near_e_bytes, cache_bytes=a.cache_bytes())), flush=True)
    recs, ref = {}, None
    for name in STATES:
        state(a, m, name)
        for k in args.nrhs:
            recs[name, k] = leg(a, lambda: a.mapping_multi_dev(X[:k], m, Out[:k]), state=name, mode=m, nrhs=k)
        if ref is None:
            ref = Out.clone()
        recs[name, "err"] = float((torch.linalg.norm(Out - ref, dim=1) / torch.linalg.norm(ref, dim=1)).max())
    for name, base in (("near", "nothing"), ("M2L + near", "M2L")):
        for k in args.nrhs:
            r, b = recs[name, k], recs[base, k]
            print(json.dumps(dict(np=args.np, mode=m, nrhs=k, state=name, against=base, ms=r["ms"], against_ms=b["ms"],
                                  pass_ratio=round(r["ms"] / b["ms"], 4), near_ms=r["near_ms"],
                                  against_near_ms=b["near_ms"], near_gain_ms=round(b["near_ms"] - r["near_ms"], 4),
                                  repeat_spread_ms=round(max(max(x["near_runs"]) - min(x["near_runs"]) for x in (r, b)), 4),
                                  stored_tb_per_s=round(nbytes * len(r["near_launches"]) / r["near_ms"] / 1e9, 3),
                                  of_achievable=round(nbytes * len(r["near_launches"]) / r["near_ms"] / 1e9 / ACHIEVABLE_TBS, 3),
                                  worst_column_vs_nothing_resident=recs[name, "err"])), flush=True)
    if args.solve > 0 and m == 0:  # main.cpp's rhs = K_0 q, on the M2L blocks without and with the near blocks
        x, y = xy[:, 0], xy[:, 1]
        Q = torch.tensor(np.array([np.exp(-w * ((x - 0.5) ** 2 + (y - 0.5) ** 2))
                                   for w in np.linspace(25.0, 100.0, args.solve)]), device="cuda")
        state(a, m, "M2L")
        solve(a, Q, "M2L blocks")
        state(a, m, "M2L + near")
        solve(a, Q, "M2L + near blocks")
    state(a, m, "nothing")
