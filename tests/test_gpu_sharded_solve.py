"""The block solve across ranks (aniso_block_solve_sharded_dev):
aniso.m's gmres(A, rhs, restart, tol, maxit) with A(u) = u - mforward(u) on a sharded
handle, every rank together.  Ranks are threads of one process on one GPU over counted,
host-staged collectives (the pattern of tests/test_gpu_sharded_passes.py); every rank's
buffers are NaN outside what it owns."""
import functools

import numpy as np
import pytest

from test_gpu_sharded_passes import _CountingCollectives, _handle, _run_ranks, _Shared, _torch

pytestmark = pytest.mark.gpu

RESTART, TOL, MAXIT = 60, 1e-11, 10


class _Ranks:
    """world sharded handles of one problem with their counting collectives; run(body)
    runs body(r, handle, collectives) on one thread per rank (the first run attaches the
    communicators)."""

    def __init__(self, sz, ks, world, coef, d=1, ml=20, lean=True):
        self.world, self.ks = world, ks
        self.hs = [_handle(sz, d, ks, ml, coef, r, world, lean=lean) for r in range(world)]
        self.shared = _Shared(world)
        self.colls = [_CountingCollectives(r, self.shared) for r in range(world)]
        self.attached = False

    def run(self, body):
        def rank(r):
            if not self.attached:
                self.hs[r].comm_init_callbacks(self.colls[r].struct)
            body(r, self.hs[r], self.colls[r])

        _run_ranks(self.world, self.shared, rank)
        self.attached = True

    def solve(self, B, X0=None, restart=RESTART, tol=TOL, maxit=MAXIT, repeat=1):
        """Every rank solves with its owned columns of B (and X0), views into buffers
        that are NaN elsewhere.  Per rank: a list (one entry per repeat) of dicts
        {iters, hist, relres, x (owned, a copy), calls}."""
        torch = _torch()
        out = [[] for _ in range(self.world)]

        def body(r, h, coll):
            b, e = h.shard()
            for _ in range(repeat):
                rhs = torch.full_like(B, float("nan"))
                rhs[:, b:e] = B[:, b:e]
                x = torch.full_like(B, float("nan"))
                x[:, b:e] = 0.0 if X0 is None else X0[:, b:e]
                n0 = len(coll.calls)
                iters, hist, relres = h.block_solve_sharded_dev(rhs[:, b:e], x[:, b:e], restart=restart, tol=tol,
                                                                maxit=maxit)
                # nothing outside the owned slices was written
                assert bool(torch.isnan(x[:, :b]).all()) and bool(torch.isnan(x[:, e:]).all())
                out[r].append(dict(iters=iters, hist=np.array(hist), relres=relres, x=x[:, b:e].clone(),
                                   calls=tuple(coll.calls[n0:])))

        self.run(body)
        return out


def _tree_rhs(N, ks, seed):
    return np.random.default_rng(seed).uniform(-1, 1, (ks, N))


def _unsharded(full, rhs_tree, x0_tree=None, restart=RESTART, tol=TOL, maxit=MAXIT):
    """The unsharded block_solve of the same system, in tree order: (iters, u, hist, relres)."""
    perm = full.tree_perm()
    rhs = np.empty_like(rhs_tree)
    rhs[:, perm] = rhs_tree  # tree[k] = orig[perm[k]]
    x0 = None
    if x0_tree is not None:
        x0 = np.empty_like(x0_tree)
        x0[:, perm] = x0_tree
    its, u, hist, relres = full.block_solve(rhs, restart=restart, tol=tol, maxit=maxit, x0=x0)
    return its, u[:, perm], hist, relres


@functools.lru_cache(maxsize=None)
def _case(sz, world, ks):
    """One problem, solved once unsharded and once (twice where asked) across ranks; the
    tests below share the results and leave them unchanged."""
    torch = _torch()
    full = _handle(sz, 1, ks, 20, None)
    rhs_tree = _tree_rhs(full.N, ks, 3)
    ref = _unsharded(full, rhs_tree)
    ranks = _Ranks(sz, ks, world, full.coef)
    B = torch.tensor(rhs_tree, device="cuda")
    res = ranks.solve(B, repeat=2 if ks == 10 else 1)
    return dict(full=full, ranks=ranks, B=B, ref=ref, res=res)


def _check_against(res, ref, what):
    """Test 1's bounds (those of the gmres_dist test, test_gpu_sharded_passes.py:372-377):
    every rank converged with the same iters / hist / relres, |iters - unsharded| <= 1,
    the concatenated solution within 1e-9."""
    torch = _torch()
    its, u, _, relres = ref
    assert its > 0 and relres <= TOL, (its, relres)
    first = [r[0] for r in res]
    for r in first:
        assert r["iters"] > 0 and r["relres"] <= TOL, (what, r["iters"], r["relres"])
        assert r["iters"] == first[0]["iters"] and r["relres"] == first[0]["relres"], what
        assert np.array_equal(r["hist"], first[0]["hist"]), what
        assert len(r["hist"]) == r["iters"]
    sol = torch.cat([r["x"] for r in first], dim=1)
    assert not bool(torch.isnan(sol).any())
    refd = torch.tensor(u, device="cuda")
    err = float(torch.linalg.norm(sol - refd) / torch.linalg.norm(refd))
    print(f"{what}: {first[0]['iters']} steps (unsharded {its}), relres {first[0]['relres']:.3e}, rel err {err:.3e}")
    assert abs(first[0]["iters"] - its) <= 1, (what, first[0]["iters"], its)
    assert err <= 1e-9, (what, err)


CASES = [(32, 2, 5), (32, 2, 10), (96, 3, 12)]  # ks <= 8; P = 2 with a padded chunk; uneven owned sizes


@pytest.mark.parametrize("sz,world,ks", CASES, ids=[f"sz{c[0]}w{c[1]}ks{c[2]}" for c in CASES])
def test_sharded_solve_matches_the_unsharded_solve(sz, world, ks):
    c = _case(sz, world, ks)
    if (sz, world) == (96, 3):
        owned = [h.n_owned() for h in c["ranks"].hs]
        assert len(set(owned)) > 1, owned
    _check_against(c["res"], c["ref"], f"sz={sz} world={world} ks={ks}")


def _ar_for(coll):
    """gmres_dist's allreduce(t) over the very collective the library calls."""
    torch = _torch()

    def red(t):
        torch.cuda.synchronize()
        assert coll._ar(None, t.data_ptr(), t.numel(), None) == 0
        return t

    return red


def _like_for_like(ranks, B, native, what):
    """The same solve through gmres_dist(kry=h) over dist.native_block_matvec and the same
    collectives: equal step count, solutions within 1e-9; the native solve's repeat is
    bitwise its first run."""
    torch = _torch()
    from aniso_amd import dist
    from aniso_amd.solve import gmres_dist

    world = ranks.world
    py = [None] * world

    def body(r, h, coll):
        b, e = h.shard()
        hist = []
        x, its, relres = gmres_dist(dist.native_block_matvec(h, ranks.ks, "cuda"), B[:, b:e].contiguous(),
                                    restart=RESTART, tol=TOL, maxit=MAXIT, allreduce=_ar_for(coll), hist=hist, kry=h)
        py[r] = (x, its, relres, np.array(hist))

    ranks.run(body)
    for r in range(world):
        a, b2 = native[r][0], native[r][1]
        assert a["iters"] == b2["iters"] and a["relres"] == b2["relres"], what
        assert np.array_equal(a["hist"], b2["hist"]) and torch.equal(a["x"], b2["x"]), f"{what}: repeat differs"
        assert py[r][1] == a["iters"] and py[r][1] > 0 and py[r][2] <= TOL, (what, py[r][1], a["iters"])
    xn = torch.cat([native[r][0]["x"] for r in range(world)], dim=1)
    xp = torch.cat([py[r][0] for r in range(world)], dim=1)
    err = float(torch.linalg.norm(xn - xp) / torch.linalg.norm(xp))
    same_x = torch.equal(xn, xp)
    same_h = np.array_equal(native[0][0]["hist"], py[0][3])
    print(f"{what}: {py[0][1]} steps both, native vs gmres_dist rel diff {err:.3e}, bitwise x {same_x}, hist {same_h}")
    assert err <= 1e-9, (what, err)


def test_like_for_like_with_gmres_dist_ks10():
    c = _case(32, 2, 10)
    _like_for_like(c["ranks"], c["B"], c["res"], "ks=10")


def test_like_for_like_with_gmres_dist_ks5_deterministic():
    torch = _torch()
    c = _case(32, 2, 5)
    ranks = _Ranks(32, 5, 2, c["full"].coef)
    for h in ranks.hs:
        h.set_deterministic(1)
    native = ranks.solve(c["B"], repeat=2)
    _like_for_like(ranks, c["B"], native, "ks=5 deterministic")
    assert torch.cat([r[0]["x"] for r in native], dim=1).shape == c["B"].shape


def test_one_rank_shard_over_rccl():
    """set_shard(0, 1) + comm_init_rccl on cached (not lean) handles at sz 64, ks 5
    (the pattern of test_native_exchange_one_rank_rccl_and_callbacks) against
    block_solve_dev: equal iters, hist allclose(1e-6, 1e-14), solution <= 1e-10 (the
    bounds of test_gpu_parity.py:1317-1319)."""
    torch = _torch()
    import aniso_amd

    ks = 5
    full = _handle(64, 1, ks, 20, None, lean=False)
    perm = torch.tensor(full.tree_perm(), device="cuda", dtype=torch.int64)
    Bt = torch.tensor(_tree_rhs(full.N, ks, 6), device="cuda")
    rhs = torch.empty_like(Bt)
    rhs[:, perm] = Bt
    x = torch.zeros_like(rhs)
    its, hist, relres = full.block_solve_dev(rhs, x, restart=RESTART, tol=TOL, maxit=MAXIT)
    assert its > 0 and relres <= TOL
    sh = _handle(64, 1, ks, 20, full.coef, 0, 1, lean=False)
    sh.comm_init_rccl(aniso_amd.comm_unique_id())
    assert sh.shard() == (0, full.N)
    xs = torch.zeros_like(Bt)
    its1, hist1, relres1 = sh.block_solve_sharded_dev(Bt, xs, restart=RESTART, tol=TOL, maxit=MAXIT)
    err = float(torch.linalg.norm(xs - x[:, perm]) / torch.linalg.norm(x))
    print(f"one rank over RCCL: {its1} steps (block_solve_dev {its}), relres {relres1:.3e}, rel err {err:.3e}")
    assert its1 == its and relres1 <= TOL
    assert np.allclose(hist1, hist, rtol=1e-6, atol=1e-14)
    assert err <= 1e-10, err


def test_collective_account_of_a_single_cycle_solve():
    """Every rank records the identical call sequence; all-reduces = 1 + 2 + 2 steps (the
    opening one, the cycle start, the confirming residual, two per step); all-to-all-v
    between P (steps + 1) and P (steps + 2) (the zero guess skips the first matvec, the
    confirming residual counts, at most one look-ahead is wasted); no all-gather in the
    one-collective form."""
    for sz, world, ks in CASES[:2]:
        c = _case(sz, world, ks)
        P = (ks + 7) // 8
        assert all(h.shard_exchange_one()["ok"] for h in c["ranks"].hs)
        for run in range(len(c["res"][0])):
            seqs = [c["res"][r][run]["calls"] for r in range(world)]
            steps = c["res"][0][run]["iters"]
            assert 0 < steps < RESTART  # one cycle
            assert all(s == seqs[0] for s in seqs)
            assert seqs[0].count("allreduce") == 1 + 2 + 2 * steps, (seqs[0].count("allreduce"), steps)
            assert P * (steps + 1) <= seqs[0].count("alltoallv") <= P * (steps + 2), (seqs[0].count("alltoallv"), steps)
            assert seqs[0].count("allgather") == 0


def test_branches_that_must_be_global():
    torch = _torch()
    sz, world, ks = 32, 2, 5
    c = _case(sz, world, ks)
    full, ranks, B = c["full"], c["ranks"], c["B"]
    b0, e0 = ranks.hs[0].shard()
    # a right-hand side that vanishes on rank 1's slice: its owner must not stop early
    B0 = torch.zeros_like(B)
    B0[:, b0:e0] = B[:, b0:e0]
    _check_against(ranks.solve(B0), _unsharded(full, B0.cpu().numpy()), "rhs on rank 0 only")
    # all zero: x = 0, iters = 0, exactly one all-reduce (and nothing else) on every rank
    X0 = torch.tensor(_tree_rhs(full.N, ks, 11), device="cuda")
    zero = ranks.solve(torch.zeros_like(B), X0=X0)
    for r in range(world):
        z = zero[r][0]
        assert z["iters"] == 0 and z["relres"] == 0.0 and z["calls"] == ("allreduce",), (z["iters"], z["calls"])
        assert float(z["x"].abs().max()) == 0.0
    # a non-zero initial guess
    _check_against(ranks.solve(B, X0=X0), _unsharded(full, B.cpu().numpy(), X0.cpu().numpy()), "x0 != 0")
    # several cycles
    multi = ranks.solve(B, restart=8, maxit=40)
    assert multi[0][0]["iters"] > 8
    _check_against(multi, _unsharded(full, B.cpu().numpy(), restart=8, maxit=40), "restart = 8")
    # not converged: the same negative count everywhere
    short = ranks.solve(B, restart=3, maxit=1)
    its = [short[r][0]["iters"] for r in range(world)]
    assert its == [-3] * world, its
    assert short[0][0]["relres"] == short[1][0]["relres"] > TOL
    assert all(short[r][0]["calls"] == short[0][0]["calls"] for r in range(world))


def test_refusals_without_hangs():
    """One rank's bad argument ends the call on every rank after exactly one all-reduce:
    the rank at fault keeps its code, the other learns that another rank refused.  Before
    comm_init, and on an unsharded handle, the error is aniso_block_op_sharded_dev's."""
    torch = _torch()
    import aniso_amd

    sz, world, ks = 32, 2, 5
    c = _case(sz, world, ks)
    ranks, B = c["ranks"], c["B"]
    got = [None] * world

    def body(r, h, coll):
        b, e = h.shard()
        x = torch.zeros(ks, e - b, dtype=torch.float64, device="cuda")
        n0 = len(coll.calls)
        try:
            h.block_solve_sharded_dev(B[:, b:e], x, restart=0 if r == 1 else 5, maxit=1)
            got[r] = None
        except aniso_amd.AnisoError as ex:
            got[r] = (ex.code, str(ex), tuple(coll.calls[n0:]), float(x.abs().max()))

    ranks.run(body)
    assert got[0] is not None and got[1] is not None, got
    assert got[1][0] == 1 and "restart >= 1" in got[1][1], got[1]
    assert got[0][0] == 1 and "another rank refused" in got[0][1], got[0]
    assert got[0][2] == got[1][2] == ("allreduce",), (got[0][2], got[1][2])
    assert got[0][3] == got[1][3] == 0.0
    # the handles still solve afterwards
    _check_against(ranks.solve(B), c["ref"], "after a refusal")

    for h in (_handle(sz, 1, ks, 20, c["full"].coef, 0, 2), c["full"]):  # before comm_init; unsharded
        own = h.n_owned()
        xs = torch.zeros(ks, own, dtype=torch.float64, device="cuda")
        xf = torch.zeros(ks, h.N, dtype=torch.float64, device="cuda")
        with pytest.raises(aniso_amd.AnisoError) as es:
            h.block_solve_sharded_dev(torch.ones_like(xs), xs, restart=5, maxit=1)
        with pytest.raises(aniso_amd.AnisoError) as eo:
            h.block_op_sharded_dev(2, xf, torch.zeros_like(xf))
        assert (es.value.code, str(es.value)) == (eo.value.code, str(eo.value))
        assert float(xs.abs().max()) == 0.0


def test_loopback_rank_runs_a_solve():
    """comm_init_loopback() on rank 1 of 4: restart = 5, maxit = 1 returns without error
    and leaves finite values (not the operator's, as in the existing loopback tests)."""
    torch = _torch()
    ks = 5
    h = _handle(64, 1, ks, 20, None, 1, 4)
    h.comm_init_loopback()
    own = h.n_owned()
    rhs = torch.tensor(np.random.default_rng(2).uniform(-1, 1, (ks, own)), device="cuda")
    x = torch.zeros_like(rhs)
    its, hist, relres = h.block_solve_sharded_dev(rhs, x, restart=5, tol=1e-300, maxit=1)
    h.sync()
    assert its == -5 and len(hist) == 5, (its, hist)
    assert bool(torch.isfinite(x).all()) and np.isfinite(hist).all() and np.isfinite(relres)
    assert float(x.abs().max()) > 0.0
