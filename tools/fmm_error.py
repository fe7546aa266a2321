"""The FMM error of a configuration, measured on the GPU against the direct evaluation
(DESIGN.md §2b "Accuracy of the method"): Aniso.fmm_error for the given modes and
Aniso.block_fmm_error for the block operator, at seeded targets, with the wall time of
each direct call and, for scale, of one mode's cache build.  One JSON line per figure.
--np 6 / 8 measures a high-order handle; for every order the last lines
give the cache sizes, the aniso_cache_block time and the block matvec's device time with
its stage spans (the M2L span as bytes/s of the stored E blocks it must read).
usage: fmm_error.py [--sz 1024] [--d 1] [--ks 5] [--ns 10] [--np 4] [--coeffs main demo]
                    [--modes 0 1 4 8] [--which 2] [--targets 256] [--seed 0]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import aniso_amd  # noqa: E402
from bench import demo_coeffs, gaussian, main_coeffs  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sz", type=int, default=1024)
ap.add_argument("--d", type=int, default=1)
ap.add_argument("--ks", type=int, default=5)
ap.add_argument("--ns", type=int, default=10)
ap.add_argument("--g", type=float, default=0.8)
ap.add_argument("--np", type=int, default=4, choices=[4, 6, 8], help="Chebyshev order per dimension")
ap.add_argument("--matvecs", type=int, default=20, help="timed block matvecs (0: skip)")
ap.add_argument("--max-level", type=int, default=20)
ap.add_argument("--coeffs", nargs="+", default=["main", "demo"], choices=["main", "demo"])
ap.add_argument("--modes", nargs="+", type=int, default=[0, 1, 4, 8])
ap.add_argument("--which", type=int, default=2)
ap.add_argument("--targets", type=int, default=256)
ap.add_argument("--seed", type=int, default=0)
args = ap.parse_args()


def timed(fn):
    """fn's result and its wall time; the host-pointer entries synchronise themselves."""
    torch.cuda.synchronize()
    t = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return r, time.perf_counter() - t


def emit(**kw):
    print(json.dumps(kw), flush=True)


for name in args.coeffs:
    a = aniso_amd.Aniso(args.sz, args.d, args.ks, args.g, args.ns, args.np, args.max_level)
    xy = a.getNodes()
    ss, st = main_coeffs(xy) if name == "main" else demo_coeffs(xy)
    a.setCoeff(ss, st)
    _, tcb = timed(a.cache_block)  # a lean handle: every mode ready, no per-mode operator
    q = ss * (gaussian(xy) + np.random.default_rng(args.seed).uniform(-0.1, 0.1, a.N))
    U = np.random.default_rng(args.seed).uniform(-1, 1, (args.ks, a.N))
    U[0] += gaussian(xy)
    tg = a.draw_targets(args.targets, args.seed)
    a.mapping_direct(q, 0, tg[:4])  # the first launch loads the code objects
    for m in args.modes:
        ref, td = timed(lambda: a.mapping_direct(q, m, tg))
        l2, mx, t = a.fmm_error(q, m, args.targets, args.seed)
        assert np.array_equal(t, tg)
        emit(coeffs=name, mode=m, rel_l2=l2, rel_max=mx, targets=int(tg.size), seed=args.seed, N=a.N,
             direct_seconds=round(td, 4))
    ref, td = timed(lambda: a.block_op_direct(args.which, U, tg))
    l2, mx, _ = a.block_fmm_error(args.which, U, args.targets, args.seed)
    emit(coeffs=name, which=args.which, rel_l2=l2, rel_max=mx, targets=int(tg.size), seed=args.seed, N=a.N,
         direct_seconds=round(td, 4))
    _, tc = timed(lambda: a.cache(0))
    _, tm = timed(lambda: a.mapping(q, 0))
    _, tm = timed(lambda: a.mapping(q, 0))
    emit(coeffs=name, np=args.np, cache_mode0_seconds=round(tc, 4), mapping_mode0_seconds=round(tm, 5))
    per_mode, shared = a.cache_bytes()
    stored = a.stats()["att_m2l_blocks"]
    e_bytes = stored * args.np ** 4 * 8  # the M2L part of the mode-shared caches
    emit(coeffs=name, np=args.np, cache_block_seconds=round(tcb, 4), cache_bytes_per_mode=per_mode,
         cache_bytes_shared=shared, stored_pairs=stored, e_block_bytes=e_bytes)
    if args.matvecs > 0:
        x = torch.tensor(U, device="cuda")
        y = torch.zeros_like(x)
        for _ in range(3):
            a.block_op_dev(2, x, y)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(args.matvecs):
            a.block_op_dev(2, x, y)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / args.matvecs
        a.set_timing(1)
        for _ in range(5):
            a.block_op_dev(2, x, y)
        st_ = a.stage_times()
        a.set_timing(0)
        emit(coeffs=name, np=args.np, block_matvec_ms=round(ms, 4), stage_ms={k: round(float(v), 4) for k, v in st_.items()},
             m2l_e_bytes_per_second=(e_bytes / (st_["m2l"] * 1e-3) if st_["m2l"] > 0 else None))
    del a
