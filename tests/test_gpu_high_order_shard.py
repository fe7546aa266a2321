"""Sharded high-order handles (np = 6, 8) on the GPU: a rank made by
aniso_create_sharded computes its own targets from the whole input, which ONE all-gather
per matvec brings into its x.  Ranks are threads of one process on one GPU, the
collectives host-staged between them and counted (the pattern of
tests/test_gpu_sharded_passes.py); every rank's input is NaN outside its own range and
its output NaN-prefilled at a row stride above N."""
import functools
import gc
import threading

import numpy as np
import pytest

from conftest import rough_coeffs

pytestmark = pytest.mark.gpu

G, NS = 0.8, 10
TOL_ROUNDING = 1e-12  # "differs by rounding only" (DESIGN.md §3.18.3): against the unsharded handle
TOL_ORACLE = 1e-10    # the project's oracle bound
# sz, d, ks, np, coefficients
SHAPES = {
    "A": (32, 1, 5, 6, "demo"),
    "B": (32, 1, 3, 8, "demo"),   # K padded to 4
    "C": (19, 3, 2, 6, "rough"),  # W and X lists
    "D": (11, 3, 2, 8, "rough"),  # W and X lists at np = 8, leaves of 12..64 points
    "T": (16, 1, 2, 8, "demo"),   # N = 256, four leaves, no M2L pair, ranks that own nothing
    "S": (32, 1, 3, 6, "demo"),   # the solve (55 steps unsharded)
    "K9": (16, 1, 9, 6, "demo"),  # more blocks than the sharded matvec holds
}
CASES = [("A", 2), ("A", 3), ("A", 4), ("B", 2), ("C", 3), ("D", 3), ("T", 8)]


def _torch():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def _coeffs(xy, coeffs):
    if coeffs == "demo":  # demo.m: sigma_s = 20, sigma_a = 0.2
        return 20.0 + 0.0 * xy[:, 0], 20.2 + 0.0 * xy[:, 0]
    return rough_coeffs(xy, 7)


def _block_ref(o, U, g, ss):
    """aniso.m forward, mforward and x - mforward(x) composed from oracle mode applies
    (as tests/test_gpu_high_order.py), the two weighted forms from one set of applies."""
    nb = U.shape[0]
    outs = []
    for which in (0, 1):
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
        outs.append(out)
    return {0: outs[0], 1: outs[1], 2: U - outs[1]}


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
    through shared slots; every call is recorded in `calls` with its count."""

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
            self.calls.append("alltoallv")  # (the np = 4 handles' exchange)
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


class _Ranks:
    """The handles of every rank of one world with their collectives attached; run(body)
    calls body(r, handle, collectives) on one thread per rank."""

    def __init__(self, shape, world, np_=None, sharded=True):
        import aniso_amd

        sz, d, ks, np0, coeffs = SHAPES[shape]
        np_ = np0 if np_ is None else np_
        self.world, self.ks = world, ks
        self.hs = []
        for r in range(world):
            if sharded:
                h = aniso_amd.Aniso(sz, d, ks, G, NS, np_, 20, shard=(r, world))
            else:
                h = aniso_amd.Aniso(sz, d, ks, G, NS, np_, 20)
                h.set_shard(r, world)
            h.setCoeff(*_coeffs(h.getNodes(), coeffs))
            h.cache_block()
            self.hs.append(h)
        self.shared = _Shared(world)
        self.colls = [_CountingCollectives(r, self.shared) for r in range(world)]
        self.run(lambda r, h, c: h.comm_init_callbacks(c.struct))

    def run(self, body):
        sh = self.shared

        def go(r):
            try:
                body(r, self.hs[r], self.colls[r])
            except Exception as ex:  # noqa: BLE001
                sh.fail(ex)

        threads = [threading.Thread(target=go, args=(r,)) for r in range(self.world)]
        for t in threads:
            t.start()
        for t in threads:
            t.join(120)
        assert not any(t.is_alive() for t in threads)
        assert not sh.errors, sh.errors


@functools.lru_cache(maxsize=None)
def _full(shape):
    """The unsharded handle of a shape, every mode ready; left as found."""
    import aniso_amd

    sz, d, ks, np_, coeffs = SHAPES[shape]
    a = aniso_amd.Aniso(sz, d, ks, G, NS, np_, 20)
    a.setCoeff(*_coeffs(a.getNodes(), coeffs))
    a.cache_block()
    return a


@functools.lru_cache(maxsize=None)
def _input(shape):
    """The (ks, N) tree-order input on the device and the unsharded handle's
    block_op_dev(which, tree=True) of it, which = 0, 1, 2."""
    torch = _torch()
    full = _full(shape)
    X = torch.tensor(np.random.default_rng(full.N + full.ks).uniform(-1, 1, (full.ks, full.N)), device="cuda")
    refs = {}
    for which in (0, 1, 2):
        refs[which] = torch.zeros_like(X)
        full.block_op_dev(which, X, refs[which], tree=True)
    torch.cuda.synchronize()
    return X, refs


@functools.lru_cache(maxsize=None)
def _oracle_refs(shape):
    """The oracle's composition of the three forms on _input(shape), in tree order."""
    from oracle.oracle_py import Oracle

    sz, d, ks, np_, coeffs = SHAPES[shape]
    full = _full(shape)
    o = Oracle(sz, d, ks, G, NS, np_, 20)
    ss, st = _coeffs(o.getNodes(), coeffs)
    o.setCoeff(ss, st)
    for m in range(2 * ks - 1):
        o.cache(m)
    perm = full.tree_perm()
    U = np.empty((ks, full.N))
    U[:, perm] = _input(shape)[0].cpu().numpy()  # tree[k] = orig[perm[k]]
    return {w: v[:, perm] for w, v in _block_ref(o, U, G, ss).items()}


@functools.lru_cache(maxsize=None)
def _case(shape, world):
    """Two block_op_sharded_dev per rank and `which`, everything the checks below read; the
    ranks stay attached for the tests that run more on them."""
    torch = _torch()
    X, _ = _input(shape)
    ks, N = X.shape
    ranks = _Ranks(shape, world)
    LD = N + 7
    rec = [dict() for _ in range(world)]

    def body(r, h, coll):
        b, e = h.shard()
        for which in (0, 1, 2):
            runs = []
            for _ in range(2):
                x = torch.full_like(X, float("nan"))
                x[:, b:e] = X[:, b:e]
                ybuf = torch.full((ks, LD), float("nan"), dtype=torch.float64, device="cuda")
                n0 = len(coll.calls)
                h.block_op_sharded_dev(which, x, ybuf)
                h.sync()
                runs.append(dict(calls=tuple(coll.calls[n0:]), y=ybuf, x=x))
            rec[r][which] = runs

    ranks.run(body)
    return dict(ranks=ranks, rec=rec)


@pytest.mark.parametrize("shape,world", CASES, ids=[f"{s}w{w}" for s, w in CASES])
def test_owned_slices_compose_the_unsharded_operator(shape, world):
    """Checks 1 and 2: the assembled owned slices against the unsharded handle (1e-12) and,
    on A, C and D, the oracle (1e-10); no NaN inside an owned slice, nothing written outside
    it; every rank's x is the whole input afterwards, bit for bit; one all-gather per
    matvec and nothing else; the second matvec returns the first's bits."""
    torch = _torch()
    X, refs = _input(shape)
    ks, N = X.shape
    c = _case(shape, world)
    hs = c["ranks"].hs
    cuts = [h.shard() for h in hs]
    assert cuts[0][0] == 0 and cuts[-1][1] == N and all(cuts[r][1] == cuts[r + 1][0] for r in range(world - 1))
    if shape == "T":
        assert [e - b for b, e in cuts] == [0, 64] * 4
    for which in (0, 1, 2):
        parts = []
        for r, (b, e) in enumerate(cuts):
            first, second = c["rec"][r][which]
            for run in (first, second):
                assert run["calls"] == ("allgather",), (r, which, run["calls"])
                assert torch.equal(run["x"], X), (r, which)
                y = run["y"]
                assert not torch.isnan(y[:, b:e]).any(), (r, which)
                assert torch.isnan(y[:, :b]).all() and torch.isnan(y[:, e:]).all(), (r, which)
            assert torch.equal(first["y"][:, b:e], second["y"][:, b:e]), (r, which)
            parts.append(first["y"][:, b:e])
        Y = torch.cat(parts, dim=1)
        err = float(torch.linalg.norm(Y - refs[which]) / torch.linalg.norm(refs[which]))
        print(f"{shape} world {world} which {which}: rel err vs unsharded {err:.3e}")
        assert err <= TOL_ROUNDING, (which, err)
        if shape in ("A", "C", "D"):
            ref = _oracle_refs(shape)[which]
            oerr = float(np.linalg.norm(Y.cpu().numpy() - ref) / np.linalg.norm(ref))
            print(f"{shape} world {world} which {which}: rel err vs oracle {oerr:.3e}")
            assert oerr <= TOL_ORACLE, (which, oerr)


@pytest.mark.parametrize("shape,world", [("A", 3), ("B", 2), ("D", 3), ("T", 8)],
                         ids=["Aw3", "Bw2", "Dw3", "Tw8"])
def test_caller_gathered_form_returns_the_same_bits(shape, world):
    """Check 3: block_op_dev(tree=True) on the whole input, no collective."""
    torch = _torch()
    X, _ = _input(shape)
    ks, N = X.shape
    c = _case(shape, world)
    for r, h in enumerate(c["ranks"].hs):
        b, e = h.shard()
        coll = c["ranks"].colls[r]
        n0 = len(coll.calls)
        for which in (0, 1, 2):
            out = torch.full((ks, max(e - b, 1) + 3), float("nan"), dtype=torch.float64, device="cuda")
            h.block_op_dev(which, X, out, tree=True)
            h.sync()
            assert torch.equal(out[:, :e - b], c["rec"][r][which][0]["y"][:, b:e]), (r, which)
            assert torch.isnan(out[:, e - b:]).all(), (r, which)
        assert len(coll.calls) == n0


def test_a_rank_holds_its_share_of_the_caches():
    """Check 4: on A at world 4 every rank's shared caches are smaller than the unsharded
    handle's, and no per-mode cache exists."""
    _torch()
    full = _full("A")
    assert full.cache_bytes()[0] == 0
    per = [h.cache_bytes() for h in _case("A", 4)["ranks"].hs]
    print(f"A world 4: shared cache bytes per rank {[p[1] for p in per]}, unsharded {full.cache_bytes()[1]}")
    for p in per:
        assert p[0] == 0 and 0 < p[1] < full.cache_bytes()[1], (p, full.cache_bytes())


@functools.lru_cache(maxsize=None)
def _solve_ref():
    """The unsharded block_solve of rhs = forward(a centred Gaussian) on shape S, in tree
    order: (steps, solution, relres, rhs)."""
    full = _full("S")
    xy = full.getNodes()
    q = np.array([np.exp(-25.0 * ((xy[:, 0] - 0.5) ** 2 + (xy[:, 1] - 0.5) ** 2)) * 0.5 ** b for b in range(full.ks)])
    rhs = full.block_op(0, q)
    its, u, _, relres = full.block_solve(rhs, restart=60, tol=1e-11, maxit=20)
    perm = full.tree_perm()
    return its, np.ascontiguousarray(u[:, perm]), relres, np.ascontiguousarray(rhs[:, perm])


@functools.lru_cache(maxsize=None)
def _solve_ranks(world):
    return _Ranks("S", world)


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_solve_matches_the_unsharded_solve(world):
    """Check 5: every rank the same iters / relres / history, converged, the assembled
    solution within 1e-8 of block_solve's; one rank's restart = 0 ends the call on every
    rank after the opening all-reduce with x untouched."""
    torch = _torch()
    import aniso_amd

    its, u, relres, rhs = _solve_ref()
    assert its > 0 and relres <= 1e-11, (its, relres)
    ranks = _solve_ranks(world)
    ks = ranks.ks
    B = torch.tensor(rhs, device="cuda")
    res = [None] * world
    bad = [None] * world
    # (an earlier test's handle that is garbage in a reference cycle is destroyed when the collector
    # next runs, and aniso_destroy, like every call, resets a thread's last error: collect now)
    gc.collect()

    def body(r, h, coll):
        b, e = h.shard()
        x = torch.zeros(ks, e - b, dtype=torch.float64, device="cuda")
        n0 = len(coll.calls)
        try:
            h.block_solve_sharded_dev(B[:, b:e], x, restart=0 if r == 1 else 60, tol=1e-11, maxit=20)
        except aniso_amd.AnisoError as ex:
            bad[r] = (ex.code, str(ex), tuple(coll.calls[n0:]), float(x.abs().max()))
        it, hist, rr = h.block_solve_sharded_dev(B[:, b:e], x, restart=60, tol=1e-11, maxit=20)
        res[r] = (it, hist, rr, x)

    ranks.run(body)
    for r in range(world):
        assert bad[r] is not None and bad[r][0] == 1 and bad[r][2] == ("allreduce",) and bad[r][3] == 0.0, bad[r]
        assert ("restart >= 1" if r == 1 else "another rank refused") in bad[r][1], bad[r]
        it, hist, rr, _ = res[r]
        assert it > 0 and rr <= 1e-11, (r, it, rr)
        assert it == res[0][0] and rr == res[0][2] and np.array_equal(hist, res[0][1]), r
    sol = torch.cat([res[r][3] for r in range(world)], dim=1)
    ref = torch.tensor(u, device="cuda")
    err = float(torch.linalg.norm(sol - ref) / torch.linalg.norm(ref))
    print(f"world {world}: sharded {res[0][0]} steps, unsharded {its}; relres {res[0][2]:.3e}; rel err {err:.3e}")
    assert err <= 1e-8, err


def test_refusals_leave_the_handle_as_it_was():
    """Check 6: what a sharded high-order handle refuses, before any launch or collective;
    a matvec afterwards returns the bits it returned before."""
    torch = _torch()
    import aniso_amd

    X, _ = _input("A")
    ks, N = X.shape
    c = _case("A", 2)
    got = [None] * 2
    gc.collect()  # (no aniso_destroy between a refused call and its message)

    def dev(*shape):
        return torch.zeros(*shape, dtype=torch.float64, device="cuda")

    def body(r, h, coll):
        b, e = h.shard()
        tg = np.arange(4, dtype=np.int64)
        refused = [
            ("tree = 0", 3, lambda: h.block_op_dev(2, X, dev(ks, N), tree=False)),
            ("mapping_dev", 3, lambda: h.mapping_dev(dev(N), 0, dev(N))),
            ("mapping_multi_dev", 3, lambda: h.mapping_multi_dev(dev(2, N), 0, dev(2, N))),
            ("block_op_multi_dev", 3, lambda: h.block_op_multi_dev(2, dev(2 * ks, N), dev(2 * ks, N))),
            ("block_op_direct", 3, lambda: h.block_op_direct(2, np.ones((ks, N)), tg)),
            ("block_op_begin_dev", 3, lambda: h.block_op_begin_dev(2, dev(ks, N), dev(ks, e - b), None)),
            ("set_deterministic", 1, lambda: h.set_deterministic(True)),
        ]
        n0 = len(coll.calls)
        codes = []
        for name, want, call in refused:
            try:
                call()
                codes.append((name, 0, ""))
            except aniso_amd.AnisoError as ex:
                codes.append((name, ex.code, str(ex)))
        ncoll = len(coll.calls) - n0
        x = torch.full_like(X, float("nan"))
        x[:, b:e] = X[:, b:e]
        y = torch.full((ks, N + 7), float("nan"), dtype=torch.float64, device="cuda")
        h.block_op_sharded_dev(2, x, y)
        h.sync()
        got[r] = (codes, [w for _, w, _ in refused], ncoll, torch.equal(y[:, b:e], c["rec"][r][2][0]["y"][:, b:e]))

    c["ranks"].run(body)
    for r in range(2):
        codes, want, ncoll, same = got[r]
        assert [k for _, k, _ in codes] == want, codes
        assert all(msg for _, _, msg in codes) and ncoll == 0 and same, (r, codes, ncoll, same)


def test_more_than_8_blocks_is_invalid_on_every_rank_before_any_collective():
    """Check 6, ks = 9: ANISO_ERR_INVALID from the matvec and from the solve, no collective."""
    torch = _torch()
    import aniso_amd

    ranks = _Ranks("K9", 2)
    got = [None] * 2

    def body(r, h, coll):
        n0 = len(coll.calls)
        b, e = h.shard()
        x = torch.zeros(9, h.N, dtype=torch.float64, device="cuda")
        xo = torch.zeros(9, e - b, dtype=torch.float64, device="cuda")
        codes = []
        for call in (lambda: h.block_op_sharded_dev(2, x, torch.zeros_like(x)),
                     lambda: h.block_op_dev(2, x, xo, tree=True),
                     lambda: h.block_solve_sharded_dev(torch.ones_like(xo), xo, restart=5, maxit=1)):
            try:
                call()
                codes.append(0)
            except aniso_amd.AnisoError as ex:
                codes.append(ex.code)
        got[r] = (codes, len(coll.calls) - n0, float(xo.abs().max()))

    ranks.run(body)
    assert got == [([1, 1, 1], 0, 0.0)] * 2, got


def test_np4_through_the_new_constructor_equals_set_shard():
    """Check 7: one world-2 matvec at np = 4 under set_deterministic(True), handles made by
    the new constructor against create + set_shard: equal bits."""
    torch = _torch()
    outs = {}
    for sharded in (True, False):
        ranks = _Ranks("A", 2, np_=4, sharded=sharded)
        N, ks = ranks.hs[0].N, ranks.ks
        X = torch.tensor(np.random.default_rng(11).uniform(-1, 1, (ks, N)), device="cuda")
        ys = [None] * 2

        def body(r, h, coll):
            h.set_deterministic(True)
            b, e = h.shard()
            x = torch.full_like(X, float("nan"))
            x[:, b:e] = X[:, b:e]
            y = torch.zeros_like(X)
            h.block_op_sharded_dev(2, x, y)
            h.sync()
            ys[r] = y[:, b:e].clone()

        ranks.run(body)
        outs[sharded] = torch.cat(ys, dim=1)
    assert not torch.isnan(outs[True]).any()
    assert torch.equal(outs[True], outs[False])
