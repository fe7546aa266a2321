"""The sharded block operator beyond 8 Fourier blocks:
aniso_block_op_sharded_dev at ks > 8 runs, per input chunk of 8 blocks, one exchange
and one up pass, and under it one window-dependent pass per output chunk.  Ranks are
threads of one process on one GPU, the collectives host-staged between them and
counted; every rank's input is NaN outside its own range."""
import threading

import numpy as np
import pytest

from conftest import rough_coeffs

pytestmark = pytest.mark.gpu

TOL = 1e-10  # against the oracle's per-mode composition (the project's bound)
G, NS, NP = 0.8, 10, 4


def _torch():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def _block_ref(o, U, g, ss, which):
    """aniso.m forward / mforward / x - mforward(x) composed from oracle mode applies
    (as tests/test_gpu_block_passes.py)."""
    nb = U.shape[0]
    out = np.zeros_like(U)
    memo = {}
    for i in range(-(nb - 1), 1):
        iid = abs(i)
        for j in range(-(nb - 1), nb):
            b, m = abs(j), abs(i - j)
            if (b, m) not in memo:
                memo[(b, m)] = o.mapping(U[b] * ss if which else U[b], m)
            w = (g ** b - g ** nb) / (1 - g ** nb) if which else 1.0
            out[iid] += w * memo[(b, m)]
    return U - out if which == 2 else out


class _Shared:
    """What the thread-ranks share: a barrier with a timeout, aborted on any rank's
    exception, so a failure ends the test instead of hanging it."""

    def __init__(self, world):
        self.world = world
        self.bar = threading.Barrier(world, timeout=60)
        self.slot = [None] * world
        self.errors = []

    def fail(self, ex):
        self.errors.append(repr(ex))
        self.bar.abort()


class _CountingCollectives:
    """aniso_collectives between handles of one process, one thread per rank, host-staged
    through shared slots (the pattern of test_native_exchange_ranks_as_threads); every
    call is recorded in `calls`."""

    def __init__(self, rank, shared):
        import aniso_amd

        self.world, self.rank, self.sh, self.lib = shared.world, rank, shared, aniso_amd
        self.calls = []
        self.struct = aniso_amd.Collectives(None, aniso_amd.COLL_ALLGATHER(self._ag),
                                            aniso_amd.COLL_ALLTOALLV(self._a2a), aniso_amd.COLL_ALLREDUCE(self._ar))

    def _host(self, ptr, n):
        buf = np.empty(int(n), dtype=np.float64)
        if n:
            self.lib.memcpy(buf.ctypes.data, ptr, 8 * int(n))
        return buf

    def _put(self, ptr, arr):
        arr = np.ascontiguousarray(arr, dtype=np.float64)
        if arr.size:
            self.lib.memcpy(ptr, arr.ctypes.data, 8 * arr.size)

    def _guard(self, fn):
        try:
            fn()
            return 0
        except Exception as ex:  # noqa: BLE001 -- the library turns the status into its error
            self.sh.fail(ex)
            return 1

    def _ag(self, ctx, send, recv, count, stream):
        def run():
            self.calls.append("allgather")
            self.sh.slot[self.rank] = self._host(send, count)
            self.sh.bar.wait()
            self._put(recv, np.concatenate([self.sh.slot[r] for r in range(self.world)]))
            self.sh.bar.wait()
        return self._guard(run)

    def _a2a(self, ctx, send, sc, so, recv, rc, ro, stream):
        def run():
            self.calls.append("alltoallv")
            self.sh.slot[self.rank] = [self._host(send + 8 * int(so[p]), int(sc[p])) for p in range(self.world)]
            self.sh.bar.wait()
            for p in range(self.world):
                if p != self.rank and int(rc[p]):
                    part = self.sh.slot[p][self.rank]
                    assert part.size == int(rc[p])
                    self._put(recv + 8 * int(ro[p]), part)
            self.sh.bar.wait()
        return self._guard(run)

    def _ar(self, ctx, buf, count, stream):
        def run():
            self.calls.append("allreduce")
            self.sh.slot[self.rank] = self._host(buf, count)
            self.sh.bar.wait()
            self._put(buf, np.sum([self.sh.slot[r] for r in range(self.world)], axis=0))
            self.sh.bar.wait()
        return self._guard(run)


def _run_ranks(world, shared, body):
    def run(r):
        try:
            body(r)
        except Exception as ex:  # noqa: BLE001
            shared.fail(ex)

    threads = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(120)
    assert not any(t.is_alive() for t in threads)
    assert not shared.errors, shared.errors


def _handle(sz, d, ks, ml, coef, rank=None, world=None, lean=True):
    import aniso_amd

    h = aniso_amd.Aniso(sz, d, ks, G, NS, NP, ml)
    if world is not None:
        h.set_shard(rank, world)
    if coef is None:  # the case's first handle: the coefficients come from its nodes
        coef = rough_coeffs(h.getNodes(), 2)
    h.coef = coef
    h.setCoeff(*coef)
    if lean:
        h.cache_block()
    else:
        for m in range(2 * ks - 1):
            h.cache(m)
    return h


# sz, d, maxLevel, world, ks, ANISO_ONE_EXCHANGE, every `which`, the form every rank must take
CASES = [
    (32, 1, 20, 2, 9, "1", True, "one"),     # smallest: P = 2, a padded chunk of 1 row; root records
    (48, 1, 20, 2, 9, "1", False, "one"),    # the upper multipoles as partial sums
    (64, 1, 20, 2, 17, "1", False, "one"),   # P = 3 (9 passes), last chunk 1 row
    (96, 1, 20, 3, 12, "1", True, "one"),    # three ranks, uneven owned sizes
    (64, 1, 20, 3, 12, "1", False, "two"),   # the cuts split a tier-0 subtree on ranks 0 and 1: all agree on two
    (64, 1, 20, 2, 12, "0", True, "two"),    # the two-collective form by request
    (40, 1, 3, 2, 9, "1", False, "two"),     # leaves above 16 points: no staged near field, k_near_hm G = 64
    (32, 2, 20, 2, 10, "1", False, "two"),   # d = 2: unfused corrections
    (128, 1, 20, 4, 12, "1", False, "one"),  # four ranks, partial sums on every rank
]


@pytest.mark.parametrize("sz,d,ml,world,ks,one_env,all_which,form", CASES,
                         ids=[f"sz{c[0]}d{c[1]}ml{c[2]}w{c[3]}ks{c[4]}one{c[5]}" for c in CASES])
def test_sharded_passes_match_the_unsharded_operator(sz, d, ml, world, ks, one_env, all_which, form, monkeypatch):
    """Owned slices of the sharded ks > 8 matvec, concatenated, against the unsharded lean
    handle's block_op_dev(tree=True): <= 1e-13 (the bound ks <= 8 is held to: only the
    summation order of the upper multipoles differs), no NaN, the second matvec bitwise
    the first; at most P all-to-all-v (and, in the two-collective form, at most P
    all-gathers) per matvec, the same sequence on every rank; the counters count
    matvecs, not chunks; the caller's x has its halo filled for all ks rows.  On the
    smallest case also against the oracle's per-mode composition (<= 1e-10)."""
    torch = _torch()
    monkeypatch.setenv("ANISO_ONE_EXCHANGE", one_env)
    P = (ks + 7) // 8
    full = _handle(sz, d, ks, ml, None)
    coef = full.coef
    N = full.N
    X = torch.tensor(np.random.default_rng(world + ks).uniform(-1, 1, (ks, N)), device="cuda")
    whiches = (2, 0, 1) if all_which else (2,)
    refs = {}
    for which in whiches:
        refs[which] = torch.zeros_like(X)
        full.block_op_dev(which, X, refs[which], tree=True)
    torch.cuda.synchronize()
    hs = [_handle(sz, d, ks, ml, coef, r, world) for r in range(world)]
    oks = [h.shard_exchange_one()["ok"] for h in hs]
    ups = [h.shard_upper_partials()["on"] for h in hs]
    staged = d == 1 and ml == 20
    one_used = one_env == "1" and all(oks) and staged
    assert ("one" if one_used else "two") == form, (oks, ups)
    shared = _Shared(world)
    colls = [_CountingCollectives(r, shared) for r in range(world)]
    outs = {w: [None] * world for w in whiches}
    per_matvec = [[] for _ in range(world)]
    halos = [None] * world

    def body(r):
        h = hs[r]
        h.comm_init_callbacks(colls[r].struct)
        b, e = h.shard()
        for which in whiches:
            x = torch.full_like(X, float("nan"))
            x[:, b:e] = X[:, b:e]
            y = torch.zeros_like(X)
            first = None
            for _ in range(2):  # the second matvec reuses the plan
                n0 = len(colls[r].calls)
                h.block_op_sharded_dev(which, x, y)
                h.sync()
                per_matvec[r].append(tuple(colls[r].calls[n0:]))
                if first is None:
                    first = y[:, b:e].clone()
            outs[which][r] = y[:, b:e].clone()
            if not torch.equal(first, outs[which][r]):
                raise AssertionError(f"rank {r}, which {which}: the second matvec differs from the first")
            if which == 2:
                rng = h.shard_one_halo() if one_used else h.shard_halo()
                halos[r] = [(int(lo), int(hi), x[:, lo:hi].clone()) for lo, hi in rng]

    _run_ranks(world, shared, body)
    for which in whiches:
        Y = torch.cat(outs[which], dim=1)
        assert not torch.isnan(Y).any(), which
        err = float(torch.linalg.norm(Y - refs[which]) / torch.linalg.norm(refs[which]))
        print(f"sz={sz} world={world} ks={ks} which={which}: rel err vs unsharded {err:.3e}")
        assert err <= 1e-13, (which, err)
    # collectives per matvec: not P^2; every rank the same sequence
    for r in range(world):
        assert per_matvec[r] == per_matvec[0], (r, per_matvec[r], per_matvec[0])
        for seq in per_matvec[r]:
            assert seq.count("alltoallv") <= P, seq
            assert seq.count("allgather") <= (0 if one_used else P), seq
            assert seq.count("allreduce") == 0, seq
    nmv = 2 * len(whiches)
    assert [h.stats()["one_exchange_applies"] for h in hs] == [nmv * int(one_used)] * world
    assert [h.stats()["upper_partial_applies"] for h in hs] == [nmv * int(one_used and all(ups))] * world
    # the halo of the caller's x, all ks rows
    for r in range(world):
        assert halos[r] is not None
        for lo, hi, got in halos[r]:
            assert torch.equal(got, X[:, lo:hi]), (r, lo, hi)
    if (sz, world, ks) == (32, 2, 9):  # independent of the unsharded GPU path
        from oracle.oracle_py import Oracle

        o = Oracle(sz, d, ks, G, NS, NP, ml)
        o.setCoeff(*coef)
        for m in range(2 * ks - 1):
            o.cache(m)
        perm = full.tree_perm()
        U = np.empty((ks, N))
        U[:, perm] = X.cpu().numpy()  # tree[k] = orig[perm[k]]
        for which in whiches:
            ref = _block_ref(o, U, G, coef[0], which)[:, perm]
            got = torch.cat(outs[which], dim=1).cpu().numpy()
            err = float(np.linalg.norm(got - ref) / np.linalg.norm(ref))
            print(f"which={which}: rel err vs oracle {err:.3e}")
            assert err <= TOL, (which, err)


def test_cached_shards_equal_lean_shards_bitwise():
    """48/2/9: handles made ready by the cache(m) loop against lean ones -- the passes
    read no per-mode operator, so the owned slices are bitwise equal."""
    torch = _torch()
    sz, d, ml, world, ks = 48, 1, 20, 2, 9
    coef = None
    res = {}
    for lean in (True, False):
        hs = []
        for r in range(world):
            hs.append(_handle(sz, d, ks, ml, coef, r, world, lean=lean))
            coef = hs[0].coef
        X = torch.tensor(np.random.default_rng(5).uniform(-1, 1, (ks, hs[0].N)), device="cuda")
        shared = _Shared(world)
        colls = [_CountingCollectives(r, shared) for r in range(world)]
        outs = [None] * world

        def body(r):
            h = hs[r]
            h.comm_init_callbacks(colls[r].struct)
            b, e = h.shard()
            x = torch.full_like(X, float("nan"))
            x[:, b:e] = X[:, b:e]
            y = torch.zeros_like(X)
            h.block_op_sharded_dev(2, x, y)
            h.sync()
            outs[r] = y[:, b:e].clone()

        _run_ranks(world, shared, body)
        res[lean] = torch.cat(outs, dim=1)
        del hs
    assert not torch.isnan(res[True]).any()
    assert torch.equal(res[True], res[False])


def test_loopback_rank_of_8_runs_the_passes(monkeypatch):
    """comm_init_loopback() on rank 3 of 8 at sz 128, ks 12: the call returns, sync()
    raises nothing and the counters move (the values are not the operator's)."""
    torch = _torch()
    monkeypatch.setenv("ANISO_ONE_EXCHANGE", "1")
    sz, ks = 128, 12
    h = _handle(sz, 1, ks, 20, None, 3, 8)
    h.comm_init_loopback()
    x = torch.tensor(np.random.default_rng(1).uniform(-1, 1, (ks, h.N)), device="cuda")
    y = torch.zeros_like(x)
    before = h.stats()
    h.block_op_sharded_dev(2, x, y)
    h.sync()
    after = h.stats()
    # every rank of 8 plans the one-collective form with partial sums (tests/test_sharded_passes_cpu.py)
    assert h.shard_exchange_one()["ok"] and h.shard_upper_partials()["on"]
    assert after["one_exchange_applies"] - before["one_exchange_applies"] == 1
    assert after["upper_partial_applies"] - before["upper_partial_applies"] == 1
    b, e = h.shard()
    assert float(y[:, b:e].abs().max()) > 0.0


def test_gmres_dist_over_the_sharded_passes_matches_the_block_solve():
    """Two thread-ranks at sz 32, ks 10: solve.gmres_dist over the one-call sharded
    operator (dist.native_block_matvec) against the unsharded block_solve of the same
    system: solution <= 1e-9, step counts within 1 (the estimate is compared at
    rounding level at the last step)."""
    torch = _torch()
    from aniso_amd import dist
    from aniso_amd.solve import gmres_dist

    sz, d, ml, world, ks = 32, 1, 20, 2, 10
    full = _handle(sz, d, ks, ml, None)
    coef = full.coef
    N = full.N
    perm = full.tree_perm()
    rhs_tree = np.random.default_rng(3).uniform(-1, 1, (ks, N))
    rhs = np.empty_like(rhs_tree)
    rhs[:, perm] = rhs_tree
    its, u, _, relres = full.block_solve(rhs, restart=60, tol=1e-11, maxit=10)
    assert its > 0 and relres <= 1e-11, (its, relres)
    ref = torch.tensor(u[:, perm], device="cuda")
    hs = [_handle(sz, d, ks, ml, coef, r, world) for r in range(world)]
    B = torch.tensor(rhs_tree, device="cuda")
    shared = _Shared(world)
    colls = [_CountingCollectives(r, shared) for r in range(world)]
    res = [None] * world

    def allreduce_for(r):
        def red(t):
            torch.cuda.synchronize()
            shared.slot[r] = t.clone()
            shared.bar.wait()
            tot = sum(shared.slot[q] for q in range(world))
            shared.bar.wait()
            t.copy_(tot)
            return t
        return red

    def body(r):
        h = hs[r]
        h.comm_init_callbacks(colls[r].struct)
        b, e = h.shard()
        apply = dist.native_block_matvec(h, ks, "cuda")
        res[r] = gmres_dist(apply, B[:, b:e].contiguous(), restart=60, tol=1e-11, maxit=10,
                            allreduce=allreduce_for(r))

    _run_ranks(world, shared, body)
    steps = [abs(r[1]) for r in res]
    assert all(r[1] > 0 and r[2] <= 1e-11 for r in res), [(r[1], r[2]) for r in res]
    assert steps[0] == steps[1] and abs(steps[0] - its) <= 1, (steps, its)
    sol = torch.cat([r[0] for r in res], dim=1)
    err = float(torch.linalg.norm(sol - ref) / torch.linalg.norm(ref))
    print(f"sharded solve: {steps[0]} steps (unsharded {its}), rel err {err:.3e}")
    assert err <= 1e-9, err


def test_what_stays_refused(monkeypatch):
    """The caller-driven two-phase form stays ANISO_ERR_INVALID for ks > 8 and points to
    aniso_block_op_sharded_dev; the one-call form before comm_init is the error it is
    at ks <= 8; without the mode-shared caches (ANISO_HARMONIC=0) both ranks get
    ANISO_ERR_INVALID before any collective."""
    torch = _torch()
    import aniso_amd

    sz, ks = 32, 9
    h = _handle(sz, 1, ks, 20, None, 0, 2)
    coef = h.coef
    x = torch.zeros(ks, h.N, dtype=torch.float64, device="cuda")
    out = torch.zeros(ks, h.n_owned(), dtype=torch.float64, device="cuda")
    ex = h.shard_exchange(8)
    roots = torch.zeros(max(ex["root_chunk"] * ex["root_record"], 1), dtype=torch.float64, device="cuda")
    with pytest.raises(aniso_amd.AnisoError) as e:
        h.block_op_begin_dev(2, x, out, roots)
    assert e.value.code == 1 and "aniso_block_op_sharded_dev" in str(e.value), str(e.value)
    small = _handle(sz, 1, 5, 20, coef, 0, 2)
    x5 = torch.zeros(5, small.N, dtype=torch.float64, device="cuda")
    with pytest.raises(aniso_amd.AnisoError) as e5:
        small.block_op_sharded_dev(2, x5, torch.zeros_like(x5))
    with pytest.raises(aniso_amd.AnisoError) as e9:
        h.block_op_sharded_dev(2, x, torch.zeros_like(x))
    assert e9.value.code == e5.value.code and str(e9.value) == str(e5.value)

    monkeypatch.setenv("ANISO_HARMONIC", "0")
    world = 2
    hs = [_handle(sz, 1, ks, 20, coef, r, world, lean=False) for r in range(world)]
    shared = _Shared(world)
    colls = [_CountingCollectives(r, shared) for r in range(world)]
    codes = [None] * world

    def body(r):
        hs[r].comm_init_callbacks(colls[r].struct)
        n0 = len(colls[r].calls)
        xx = torch.zeros(ks, hs[r].N, dtype=torch.float64, device="cuda")
        try:
            hs[r].block_op_sharded_dev(2, xx, torch.zeros_like(xx))
            codes[r] = 0
        except aniso_amd.AnisoError as ex:
            codes[r] = (ex.code, len(colls[r].calls) - n0)

    _run_ranks(world, shared, body)
    assert codes == [(1, 0)] * world, codes
