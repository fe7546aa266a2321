"""Resident mode operators of a high-order handle, timed: mode 0's pass
and its M2L span at 1, 8 and 16 columns through the mode kernels (k_ho_m2l_mode) and through
the resident blocks (cache_mode(0): the fp64 MFMA M2L of mode_resident.hip), in one process
on one handle; the build of the blocks; the resident M2L's bytes over its span (the stored
bytes, and what the launch reads: a stored V pair is read from both of its ends); and an
8-source forward solve both ways.  Every leg: 20 calls between two events after 3 warm-ups,
repeated --repeats times (median and spread), then its stage spans from aniso_set_timing(1)
over 5 more calls.  The headline geometry by default.  One JSON line per leg.
usage: mode_resident_time.py --np 6 [--sz 1024] [--d 1] [--ks 5] [--ns 10] [--mode 0]
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
ap.add_argument("--mode", type=int, default=0)
ap.add_argument("--nrhs", nargs="+", type=int, default=[1, 8, 16])
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--solve", type=int, default=8, help="sources of the forward solve (0: none)")
args = ap.parse_args()

ACHIEVABLE_TBS, K64_M2L_TBS = 6.3, 5.5  # the stream rate HBM sustains; what k64_m2l reached


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
    rec = dict(leg=name, np=args.np, N=a.N, ms=round(ms, 4), runs=[round(r, 4) for r in runs],
               spread=round((max(runs) - min(runs)) / ms, 5), passes=a.mode_apply_calls().tolist(),
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
        print(json.dumps(dict(leg="forward_solve_multi_dev", route=label, sources=int(Q.shape[0]), run=rep,
                              wall_s=round(wall, 4), iters=iters.tolist(), relres=relres.tolist(),
                              operator_calls=len(a.forward_solve_calls()),
                              last_passes=a.mode_apply_calls().tolist())), flush=True)


a = aniso_amd.Aniso(args.sz, args.d, args.ks, args.g, args.ns, args.np, args.max_level)
xy = a.getNodes()
a.setCoeff(*main_coeffs(xy))
a.cache_block()
m = args.mode
rng = np.random.default_rng(0)
nmax = max(args.nrhs)
X = torch.tensor(rng.uniform(-1, 1, (nmax, a.N)) + gaussian(xy), device="cuda")
Out = torch.zeros_like(X)
Q = None
if args.solve > 0:  # main.cpp's rhs = K_0 q
    x, y = xy[:, 0], xy[:, 1]
    Q = torch.tensor(np.array([np.exp(-w * ((x - 0.5) ** 2 + (y - 0.5) ** 2))
                               for w in np.linspace(25.0, 100.0, args.solve)]), device="cuda")

plain = {k: leg(a, "mapping_multi_dev", lambda: a.mapping_multi_dev(X[:k], m, Out[:k]), route="mode kernels",
                mode=m, nrhs=k) for k in args.nrhs}
ref = Out.clone()
if Q is not None and m == 0:
    solve(a, Q, "mode kernels")

torch.cuda.synchronize()
t = time.perf_counter()
a.cache_mode(m)
build_s = time.perf_counter() - t
nbytes = a.cache_mode_bytes()
st = a.stats()
# what one M2L launch reads: a stored V pair once from each end (m2l_pairs: the list entries)
read_bytes = nbytes // max(st["att_m2l_blocks"], 1) * st["m2l_pairs"]
print(json.dumps(dict(leg="cache_mode", np=args.np, mode=m, wall_s=round(build_s, 4), bytes=nbytes,
                      stored_blocks=st["att_m2l_blocks"], block_reads=st["m2l_pairs"], read_bytes=read_bytes,
                      cache_bytes=a.cache_bytes())), flush=True)

for k in args.nrhs:
    r = leg(a, "mapping_multi_dev", lambda: a.mapping_multi_dev(X[:k], m, Out[:k]), route="resident", mode=m, nrhs=k)
    span, old = r["stage_ms"]["m2l"], plain[k]["stage_ms"]["m2l"]
    npass = len(plain[k]["passes"])  # (stage spans are means per pass: 16 columns are two passes of the mode kernels)
    err = float((torch.linalg.norm(Out[:k] - ref[:k], dim=1) / torch.linalg.norm(ref[:k], dim=1)).max())
    print(json.dumps(dict(mode=m, nrhs=k, ms=r["ms"], mode_kernels_ms=plain[k]["ms"],
                          pass_ratio=round(r["ms"] / plain[k]["ms"], 4), m2l_ms=span, mode_kernels_m2l_ms=round(old * npass, 4),
                          m2l_ratio=round(span / (old * npass), 4) if old > 0 else None,
                          stored_tb_per_s=round(nbytes / span / 1e9, 3) if span > 0 else None,
                          read_tb_per_s=round(read_bytes / span / 1e9, 3) if span > 0 else None,
                          of_achievable=round(read_bytes / span / 1e9 / ACHIEVABLE_TBS, 3) if span > 0 else None,
                          of_k64_m2l=round(read_bytes / span / 1e9 / K64_M2L_TBS, 3) if span > 0 else None,
                          spread=max(r["spread"], plain[k]["spread"]), worst_column_vs_mode_kernels=err)), flush=True)
if Q is not None and m == 0:
    solve(a, Q, "resident")
a.cache_mode_free()
