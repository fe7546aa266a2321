"""One rank of a sharded high-order block matvec, timed on one GPU: a handle
made by aniso_create_sharded at np = 6 and np = 8 with the loopback communicator, which
moves the rank's own part of the all-gather only -- the caller supplies the whole input, so
the rank's launches are those of an N-GPU run and its values are the operator's; the
collective itself (over xGMI) is NOT in these figures.  Legs: ranks 0, 3 and 5 of 8 and rank
0 of 2.  Yardstick: block_op_dev(2) of the unsharded handle of the same order in the same
process.  Every leg: 20 calls between two events after 3 warm-ups, repeated 3 times (median
and spread), then its stage spans from aniso_set_timing(1) over 5 more calls (exchange = the
pack kernel, gather = the unpack kernel on these handles) and the rank's aniso_cache_bytes
against the unsharded handle's.  The headline geometry by default.  One JSON line per result.
Manual: no test and no benchmark runs it.
usage: high_shard_time.py [--np 6 8] [--legs 0/8 3/8 5/8 0/2] [--sz 1024] [--d 1] [--ks 5] [--ns 10]
                          [--calls 20] [--repeats 3]"""
import argparse
import json
import os
import sys

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
ap.add_argument("--np", nargs="+", type=int, default=[6, 8], choices=[6, 8], help="Chebyshev orders per dimension")
ap.add_argument("--max-level", type=int, default=20)
ap.add_argument("--legs", nargs="+", default=["0/8", "3/8", "5/8", "0/2"], help="rank/nranks")
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--repeats", type=int, default=3)
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


def leg(a, fn):
    """(median ms, spread, the repeats, the stage spans) of a leg."""
    for _ in range(3):
        fn()
    ms = [timed(fn, args.calls) for _ in range(args.repeats)]
    a.set_timing(1)
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    st = a.stage_times()
    a.set_timing(0)
    spans = dict(m2l_ms=st["m2l"], near_ms=st["near"], corr_ms=st["corr"], up_ms=st["up"], down_ms=st["down"],
                 pack_ms=st["exchange"], unpack_ms=st["gather"], apply_ms=st["total"])
    return float(np.median(ms)), max(ms) - min(ms), ms, {k: round(float(v), 4) for k, v in spans.items()}


def handle(np_, shard=None):
    a = aniso_amd.Aniso(args.sz, args.d, args.ks, args.g, args.ns, np_, args.max_level, shard=shard)
    a.setCoeff(*main_coeffs(a.getNodes()))
    a.cache_block()
    return a


for np_ in args.np:
    full = handle(np_)
    N, ks = full.N, full.ks
    X = torch.tensor(np.random.default_rng(0).uniform(-1, 1, (ks, N)), device="cuda")  # tree order
    ref = torch.zeros_like(X)
    yard, yspread, yms, yspans = leg(full, lambda: full.block_op_dev(2, X, ref, tree=True))
    full_bytes = full.cache_bytes()[1]
    print(json.dumps(dict(leg="unsharded block_op_dev(2)", np=np_, N=N, ks=ks, ms=round(yard, 4),
                          spread_ms=round(yspread, 4), repeats=[round(m, 4) for m in yms], cache_bytes=full_bytes,
                          **yspans)), flush=True)
    for spec in args.legs:
        rank, world = (int(v) for v in spec.split("/"))
        h = handle(np_, shard=(rank, world))
        h.comm_init_loopback()
        b, e = h.shard()
        x = X.clone()  # the loopback moves the own part only: the whole input is the caller's
        y = torch.zeros_like(X)
        ms, spread, rep, spans = leg(h, lambda: h.block_op_sharded_dev(2, x, y))
        err = float(torch.linalg.norm(y[:, b:e] - ref[:, b:e]) / torch.linalg.norm(ref[:, b:e])) if e > b else 0.0
        st = h.stats()
        print(json.dumps(dict(leg=f"rank {rank} of {world}", np=np_, owned=e - b, ms=round(ms, 4),
                              spread_ms=round(spread, 4), repeats=[round(m, 4) for m in rep],
                              over_unsharded=round(ms / yard, 4), unsharded_ms=round(yard, 4),
                              m2l_targets=st["m2l_targets"], stored_blocks=st["att_m2l_blocks"],
                              cache_bytes=h.cache_bytes()[1], cache_over_unsharded=round(h.cache_bytes()[1] / full_bytes, 4),
                              gathered_doubles_received=ks * (N - (e - b)), owned_vs_unsharded=err, **spans)),
              flush=True)
        del h, x, y
        torch.cuda.empty_cache()
    del full, X, ref
    torch.cuda.empty_cache()
