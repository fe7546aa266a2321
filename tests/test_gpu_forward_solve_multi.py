"""The multi-source forward solve on the GPU: forward_solve_multi_dev
and forward_solve_multi -- main.cpp:121-141 for several sources, every column a restarted
GMRES of its own over forward_multi_dev's routes -- against the CPU oracle's gmres_main at
the same order on np = 6 and 8 handles, and on np = 4 handles, lean and resident.

Step counts are compared with the reference's only for columns that clear tol by at least
1 %: the reference's last estimate above tol is >= 1.01 tol and its first below is <= 0.99
tol (100x the rtol = 1e-4 at which test_forward_operator_and_gmres_match_reference holds
the two histories together).  Measured with the oracle at tol 1e-12: S1 mixed, restart 80:
23, 36, 35, 25, 36, 28 steps, every column clears the margin (closest: 1.156e-12 above);
S1 random, restart 80: 36 steps each, all clear (closest 1.105e-12); S1 random, restart 8:
66, 93, 82, 94, 68, 72, 102, 94, 97, 96, 77 steps, columns 3 (9.957e-13 below) and 8
(1.0028e-12 above) miss the margin and are left out of the count comparison only; S2
random, restart 80: 17 steps each, all clear."""
import functools

import numpy as np
import pytest

from conftest import gaussian_charge, main_coeffs, rough_coeffs

pytestmark = pytest.mark.gpu

TOL = 1e-12   # main.cpp:141
XTOL = 1e-10  # the suite's oracle-parity bound on a solution
G = 0.8

# np, sz, d, ks, ns, maxLevel, coefficients
S1 = (6, 32, 1, 3, 10, 20, "main")    # N 1024
S2 = (8, 11, 3, 2, 8, 20, "rough")    # N 1089: W and X lists, leaves of 12..64 points
S3 = (4, 16, 1, 2, 8, 20, "main")     # N 256: lean (cache_block) and resident (cache(0))


def _torch():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def _rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def _coeffs(xy, coeffs):
    return main_coeffs(xy) if coeffs == "main" else rough_coeffs(xy, 7)


@functools.lru_cache(maxsize=None)
def _handle(shape, how="block"):
    """A device handle with mode 0 ready: "block" (aniso_cache_block) or "mode0"
    (aniso_cache(0)).  Built once per shape, left as found."""
    import aniso_amd

    np_, sz, d, ks, ns, ml, coeffs = shape
    a = aniso_amd.Aniso(sz, d, ks, G, ns, np_, ml)
    a.setCoeff(*_coeffs(a.getNodes(), coeffs))
    if how == "block":
        a.cache_block()
    else:
        a.cache(0)
    return a


@functools.lru_cache(maxsize=None)
def _oracle(shape):
    from oracle.oracle_py import Oracle

    np_, sz, d, ks, ns, ml, coeffs = shape
    o = Oracle(sz, d, ks, G, ns, np_, ml)
    o.setCoeff(*_coeffs(o.getNodes(), coeffs))
    o.cache(0)
    return o


@functools.lru_cache(maxsize=None)
def _columns(shape, kind):
    xy = _oracle(shape).getNodes()
    N = xy.shape[0]
    rng = np.random.default_rng(11 + N)
    if kind == "random":
        Q = rng.uniform(-1.0, 1.0, (11, N))
    else:  # "mixed"
        x, y = xy[:, 0], xy[:, 1]
        Q = np.array([gaussian_charge(xy), rng.uniform(-1.0, 1.0, N),
                      np.exp(-200.0 * ((x - 0.2) ** 2 + (y - 0.7) ** 2)), np.ones(N),
                      1e-3 * rng.uniform(-1.0, 1.0, N), (x > 0.5).astype(np.float64)])
    Q.setflags(write=False)
    return Q


@functools.lru_cache(maxsize=None)
def _oracle_solve(shape, kind, j, restart):
    """gmres_main(q, restart, 400, tol) of column j: (steps, x, history)."""
    it, x, h, _ = _oracle(shape).gmres_main(_columns(shape, kind)[j], restart, 400, TOL)
    x.setflags(write=False)
    h.setflags(write=False)
    return it, x, h


def _clears(h, it):
    """The reference history h (h[k]: the residual after k steps) clears tol at step `it`
    by at least 1 % on both sides."""
    return it > 0 and h[it - 1] >= 1.01 * TOL and h[it] <= 0.99 * TOL


def _rows(torch, X, pad=7, extra=0, fill=float("nan")):
    """X's rows in a (rows + extra, N + pad) tensor filled with `fill`; returns the whole
    tensor and the view of the first rows."""
    k, N = X.shape
    t = torch.full((k + extra, N + pad), fill, dtype=torch.float64, device="cuda")
    t[:k, :N] = torch.tensor(X, device="cuda")
    return t, t[:k]


# ---- 1. oracle parity, one cycle

@pytest.mark.parametrize("shape,picks", [(S1, [("mixed", j) for j in range(6)] + [("random", j) for j in range(5)]),
                                         (S2, [("random", j) for j in range(5)])], ids=["S1", "S2"])
def test_every_column_matches_the_oracle(shape, picks):
    """restart 80, maxit 5, rhs_is_source: rows at stride N + 7 with NaN in the gaps, two
    rows behind the columns.  Every column: solution <= 1e-10 from gmres_main's, the same
    step count (under the rule; every column here clears the margin), relres <= tol and the
    estimates after each step against the oracle's history (rtol 1e-4, atol 1e-15)."""
    torch = _torch()
    a = _handle(shape)
    N = a.N
    Q = np.array([_columns(shape, kind)[j] for kind, j in picks])
    n = len(picks)
    qwhole, Qd = _rows(torch, Q, extra=2)
    qwhole[n:] = 5.0
    xwhole, Xd = _rows(torch, np.zeros((n, N)), extra=2)
    xwhole[n:] = 7.0
    iters, relres, hist = a.forward_solve_multi_dev(Qd, Xd, restart=80, tol=TOL, maxit=5, rhs_is_source=True)
    torch.cuda.synchronize()
    got = xwhole.cpu().numpy()
    assert np.all(np.isnan(got[:n, N:])) and np.all(got[n:] == 7.0)
    qgot = qwhole.cpu().numpy()
    assert np.all(np.isnan(qgot[:n, N:])) and np.all(qgot[n:] == 5.0) and np.array_equal(qgot[:n, :N], Q)
    compared = 0
    for c, (kind, j) in enumerate(picks):
        it, xo, ho = _oracle_solve(shape, kind, j, 80)
        err = _rel(got[c, :N], xo)
        print(f"np {shape[0]} {kind} {j}: {iters[c]} steps (oracle {it}), relres {relres[c]:.3e}, x vs oracle {err:.3e}, "
              f"oracle above {ho[it - 1]:.4e} below {ho[it]:.4e}")
        assert err <= XTOL, (c, err)
        assert iters[c] > 0 and relres[c] <= TOL, (c, iters[c], relres[c])
        if _clears(ho, it):
            compared += 1
            assert iters[c] == it, (c, iters[c], it)
        m = min(int(iters[c]), it)
        np.testing.assert_allclose(hist[c, :m], ho[1:m + 1], rtol=1e-4, atol=1e-15)
        assert np.all(hist[c, iters[c]:] == 0.0)
    assert compared >= n - 2, compared


# ---- 2. several cycles, columns finishing in different cycles

def test_restart_8_columns_finish_in_different_cycles():
    """S1, the 11 random columns, restart 8, maxit 60 (the oracle takes 66 .. 102 steps, 9
    to 13 cycles): solutions <= 1e-10 from gmres_main(q, 8, 400, tol), step counts under the
    rule (columns 3 and 8 miss the margin)."""
    torch = _torch()
    a = _handle(S1)
    N = a.N
    Q = _columns(S1, "random")
    Qd = torch.tensor(Q, device="cuda")
    Xd = torch.zeros(11, N, dtype=torch.float64, device="cuda")
    iters, relres, _ = a.forward_solve_multi_dev(Qd, Xd, restart=8, tol=TOL, maxit=60)
    torch.cuda.synchronize()
    got = Xd.cpu().numpy()
    compared = 0
    for c in range(11):
        it, xo, ho = _oracle_solve(S1, "random", c, 8)
        err = _rel(got[c], xo)
        print(f"restart 8 column {c}: {iters[c]} steps (oracle {it}), relres {relres[c]:.3e}, x vs oracle {err:.3e}, "
              f"oracle above {ho[it - 1]:.4e} below {ho[it]:.4e}")
        assert err <= XTOL, (c, err)
        assert iters[c] > 0 and relres[c] <= TOL, (c, iters[c], relres[c])
        if _clears(ho, it):
            compared += 1
            assert iters[c] == it, (c, iters[c], it)
    assert compared >= 9, compared
    assert len({(abs(int(i)) - 1) // 8 for i in iters}) > 1  # they did finish in different cycles


# ---- 3. not converged, and a column frozen from the start

def test_not_converged_and_a_zero_column():
    """S3 lean, 4 random columns and an all-zero one (in the middle), restart 8, maxit 3:
    GMRES(8) stagnates there (the oracle is still at 1e-2 .. 1e-1 after 400 steps).  Every
    nonzero column: iters = -24, relres < 1 and within a relative 1e-6 of |b - A x| / |b|
    from the oracle's mapping on the returned x (the operators agree to 1e-10 and the
    residual is >= 1e-2: 1e-8, and 100x for the restart-8 cycle).  The zero column: x = 0,
    iters = 0, relres = 0."""
    torch = _torch()
    a = _handle(S3)
    assert a.cache_bytes()[0] == 0
    N = a.N
    o = _oracle(S3)
    ss, _ = _coeffs(o.getNodes(), "main")
    Q = np.zeros((5, N))
    Q[[0, 1, 3, 4]] = _columns(S3, "random")[:4]
    Xd = torch.full((5, N), 0.0, dtype=torch.float64, device="cuda")
    Xd[2] = 3.0  # a guess the zero column must overwrite
    iters, relres, hist = a.forward_solve_multi_dev(torch.tensor(Q, device="cuda"), Xd, restart=8, tol=TOL, maxit=3)
    torch.cuda.synchronize()
    got = Xd.cpu().numpy()
    assert iters[2] == 0 and relres[2] == 0.0 and np.all(got[2] == 0.0) and np.all(hist[2] == 0.0)
    for c in (0, 1, 3, 4):
        b = o.mapping(Q[c], 0)
        r = b - (got[c] - o.mapping(ss * got[c], 0))
        ref = float(np.linalg.norm(r) / np.linalg.norm(b))
        print(f"stagnating column {c}: iters {iters[c]}, relres {relres[c]:.6e}, oracle's residual of x {ref:.6e}")
        assert iters[c] == -24, (c, iters[c])
        assert relres[c] < 1.0 and ref >= 1e-2, (c, relres[c], ref)
        assert abs(relres[c] - ref) <= 1e-6 * ref, (c, relres[c], ref)
        assert np.all(hist[c, :24] > 0.0)


# ---- 4. initial guess and rhs_is_source = 0

def test_initial_guess_and_a_given_right_hand_side():
    torch = _torch()
    a = _handle(S2)
    N = a.N
    Q = _columns(S2, "random")[:3]
    Qd = torch.tensor(Q, device="cuda")
    guess = np.random.default_rng(3).uniform(-1.0, 1.0, (3, N))
    Xg = torch.tensor(guess, device="cuda")
    iters, relres, _ = a.forward_solve_multi_dev(Qd, Xg, restart=80, tol=TOL, maxit=5)
    torch.cuda.synchronize()
    for c in range(3):
        err = _rel(Xg[c].cpu().numpy(), _oracle_solve(S2, "random", c, 80)[1])
        print(f"from a random guess, column {c}: {iters[c]} steps, relres {relres[c]:.3e}, x vs oracle {err:.3e}")
        assert iters[c] > 0 and relres[c] <= TOL and err <= XTOL, (c, iters[c], relres[c], err)
    X1 = torch.zeros(3, N, dtype=torch.float64, device="cuda")
    it1, rr1, h1 = a.forward_solve_multi_dev(Qd, X1, restart=80, tol=TOL, maxit=5, rhs_is_source=True)
    Bd = torch.zeros(3, N, dtype=torch.float64, device="cuda")
    a.mapping_multi_dev(Qd, 0, Bd)
    X0 = torch.zeros(3, N, dtype=torch.float64, device="cuda")
    it0, rr0, h0 = a.forward_solve_multi_dev(Bd, X0, restart=80, tol=TOL, maxit=5, rhs_is_source=False)
    torch.cuda.synchronize()
    assert np.array_equal(it0, it1)
    for c in range(3):
        err = _rel(X0[c].cpu().numpy(), X1[c].cpu().numpy())
        assert err <= 1e-12, (c, err)


# ---- 5. columns are independent; calls repeat bitwise

def test_columns_are_independent_and_calls_repeat_bitwise():
    """S1 mixed (23 .. 36 steps): column k alone against the 6-column call (equal steps under
    the rule, solutions <= 1e-10); the 6-column call twice: equal bits; and its operator calls
    shrink as the columns freeze: step j runs on exactly the columns with more than j steps,
    and one call on all six gives the explicit residuals."""
    torch = _torch()
    a = _handle(S1)
    N = a.N
    Q = _columns(S1, "mixed")
    Qd = torch.tensor(Q, device="cuda")
    X6 = torch.zeros(6, N, dtype=torch.float64, device="cuda")
    it6, rr6, h6 = a.forward_solve_multi_dev(Qd, X6, restart=80, tol=TOL, maxit=5)
    calls = list(a.forward_solve_calls())
    again = torch.zeros(6, N, dtype=torch.float64, device="cuda")
    it6b, rr6b, h6b = a.forward_solve_multi_dev(Qd, again, restart=80, tol=TOL, maxit=5)
    torch.cuda.synchronize()
    assert torch.equal(X6, again)
    assert np.array_equal(it6, it6b) and np.array_equal(rr6, rr6b) and np.array_equal(h6, h6b)
    assert np.all(it6 > 0) and len(set(it6.tolist())) > 1, it6
    assert calls == [int((it6 > j).sum()) for j in range(int(it6.max()))] + [6], (calls, it6)
    for c in range(6):
        X1 = torch.zeros(1, N, dtype=torch.float64, device="cuda")
        it1, rr1, _ = a.forward_solve_multi_dev(Qd[c:c + 1], X1, restart=80, tol=TOL, maxit=5)
        torch.cuda.synchronize()
        err = _rel(X1[0].cpu().numpy(), X6[c].cpu().numpy())
        it, _, ho = _oracle_solve(S1, "mixed", c, 80)
        print(f"column {c} alone: {it1[0]} steps ({it6[c]} among six), x alone vs among six {err:.3e}")
        assert rr1[0] <= TOL and err <= XTOL, (c, rr1[0], err)
        if _clears(ho, it):
            assert it1[0] == it6[c], (c, it1[0], it6[c])


# ---- 6. np = 4 resident against the existing solve

def test_order_4_resident_matches_aniso_gmres():
    torch = _torch()
    a = _handle(S3, "mode0")
    N = a.N
    Q = _columns(S3, "random")[:3]
    X = torch.zeros(3, N, dtype=torch.float64, device="cuda")
    iters, relres, _ = a.forward_solve_multi_dev(torch.tensor(Q, device="cuda"), X, restart=80, tol=TOL, maxit=5)
    torch.cuda.synchronize()
    for c in range(3):
        it, x, h, _ = a.gmres(Q[c], 80, 400, TOL)
        err = _rel(X[c].cpu().numpy(), x)
        print(f"np 4 resident column {c}: {iters[c]} steps (aniso_gmres {it}), relres {relres[c]:.3e}, x {err:.3e}, "
              f"gmres above {h[it - 1]:.4e} below {h[it]:.4e}")
        assert it > 0 and iters[c] > 0 and relres[c] <= TOL and err <= XTOL, (c, it, iters[c], relres[c], err)
        if _clears(h, it):
            assert iters[c] == it, (c, iters[c], it)


# ---- 7. the host entry, what is left behind, and a mode that is not ready

def test_host_entry_and_what_is_left_behind():
    torch = _torch()
    a = _handle(S2)
    N, ks = a.N, a.ks
    U = np.random.default_rng(5).uniform(-1.0, 1.0, (ks, N))
    first = a.block_op(2, U)
    Q = _columns(S2, "random")[:3]
    Xh, ith, rrh = a.forward_solve_multi(Q.T, restart=80, tol=TOL, maxit=5)
    assert Xh.shape == (N, 3)
    X = torch.zeros(3, N, dtype=torch.float64, device="cuda")
    iters, relres, _ = a.forward_solve_multi_dev(torch.tensor(Q, device="cuda"), X, restart=80, tol=TOL, maxit=5)
    torch.cuda.synchronize()
    assert np.array_equal(ith, iters) and np.array_equal(rrh, relres)
    for c in range(3):
        assert _rel(Xh[:, c], X[c].cpu().numpy()) <= 1e-15, c
    assert np.array_equal(a.block_op(2, U), first)
    assert a.cache_bytes()[0] == 0


def test_before_mode_0_is_ready_is_a_state_error_that_names_aniso_cache():
    torch = _torch()
    import aniso_amd

    for np_ in (4, 6):
        a = aniso_amd.Aniso(8, 1, 2, 0.5, 6, np_, 20)
        a.setCoeff(np.ones(a.N), 1.2 * np.ones(a.N))
        q = torch.zeros(2, a.N, dtype=torch.float64, device="cuda")
        with pytest.raises(aniso_amd.AnisoError) as e:
            a.forward_solve_multi_dev(q, torch.zeros_like(q))
        assert e.value.code == 3 and "aniso_cache" in str(e.value), (np_, str(e.value))
