"""The block operator and its solve for several sources on the GPU:
block_op_multi(_dev) against block_op_dev of the same handle and against the CPU oracle,
the independence of a source's bits from the call around it (property P), and
block_solve_multi(_dev) against block_solve per source."""
import functools

import numpy as np
import pytest

from conftest import main_coeffs, rough_coeffs

pytestmark = pytest.mark.gpu

G = 0.8
PARITY = 1e-12  # the project's bound for the same operator on another route (test_gpu_mode_multi.py)
ORACLE = 1e-10  # the suite's oracle-parity bound
TOL = 1e-11     # aniso.m:162
NSRC = (1, 2, 3, 4, 5, 7)

# sz, d, ks, ns, coefficients, np, how the modes are made ready
A = (32, 1, 5, 10, "demo", 6, "block")   # K = 5
B = (32, 1, 3, 10, "demo", 8, "block")   # K padded to 4, 64-point leaves
C = (19, 3, 2, 8, "rough", 6, "block")   # W and X lists, K = 2
D = (16, 1, 8, 10, "main", 6, "block")   # K = 8
E = (32, 1, 9, 10, "demo", 6, "block")   # ks > 8: one block_op_dev per source
F = (16, 1, 3, 10, "demo", 4, "modes")   # np = 4 cached: one block_op_dev per source
FL = (16, 1, 3, 10, "demo", 4, "block")  # np = 4 lean
A3 = (32, 1, 3, 10, "demo", 6, "block")  # the shape of test_block_solve_converges_to_the_oracle_operator


def _torch():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def _rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def _coeffs(xy, coeffs):
    if coeffs == "demo":  # demo.m: sigma_s = 20, sigma_a = 0.2
        return 20.0 + 0.0 * xy[:, 0], 20.2 + 0.0 * xy[:, 0]
    return main_coeffs(xy) if coeffs == "main" else rough_coeffs(xy, 7)


@functools.lru_cache(maxsize=None)
def _handle(shape):
    """A device handle with every mode ready.  Built once per shape, left as found.  An np = 4
    handle is made deterministic: its default clustered M2L sums with
    atomics, so two block_op_dev calls differ in the last bits and no bitwise comparison with
    that call could hold; np = 6, 8 sum in a fixed order as they are."""
    import aniso_amd

    sz, d, ks, ns, coeffs, np_, how = shape
    a = aniso_amd.Aniso(sz, d, ks, G, ns, np_, 20)
    a.setCoeff(*_coeffs(a.getNodes(), coeffs))
    if how == "block":
        a.cache_block()
    else:
        for m in range(2 * ks - 1):
            a.cache(m)
    if np_ == 4:
        a.set_deterministic(True)
    return a


@functools.lru_cache(maxsize=None)
def _oracle(shape):
    from oracle.oracle_py import Oracle

    sz, d, ks, ns, coeffs, np_, _ = shape
    o = Oracle(sz, d, ks, G, ns, np_, 20)
    o.setCoeff(*_coeffs(o.getNodes(), coeffs))
    for m in range(2 * ks - 1):
        o.cache(m)
    return o


@functools.lru_cache(maxsize=None)
def _sources(shape):
    """Seven sources of ks blocks, uniform in (-1, 1): (7, ks, N)."""
    a = _handle(shape)
    U = np.random.default_rng(100 + a.ks + a.N).uniform(-1.0, 1.0, (7, a.ks, a.N))
    U.setflags(write=False)
    return U


@functools.lru_cache(maxsize=None)
def _single(shape, which):
    """block_op_dev of every source on the same handle: (7, ks, N)."""
    torch = _torch()
    a = _handle(shape)
    out = np.zeros_like(_sources(shape))
    for s, U in enumerate(_sources(shape)):
        o = torch.zeros(a.ks, a.N, dtype=torch.float64, device="cuda")
        a.block_op_dev(which, torch.tensor(U, device="cuda"), o)
        torch.cuda.synchronize()
        out[s] = o.cpu().numpy()
    out.setflags(write=False)
    return out


def _rows(torch, X, pad=7):
    """The rows of X (rows, N) in a (rows, N + pad) tensor with NaN in the gaps: the whole
    tensor and the view of the first N columns."""
    k, N = X.shape
    t = torch.full((k, N + pad), float("nan"), dtype=torch.float64, device="cuda")
    t[:, :N] = torch.tensor(X, device="cuda")
    return t, t[:, :N]


def _multi(a, which, U):
    """block_op_multi_dev of the sources U (n, ks, N) at row stride N + 7, NaN in the gaps of
    input and output; the gaps must stay NaN and the input as it was.  Returns (n, ks, N)."""
    torch = _torch()
    n, ks, N = U.shape
    xw, X = _rows(torch, U.reshape(n * ks, N))
    ow, Out = _rows(torch, np.zeros((n * ks, N)))
    a.block_op_multi_dev(which, X, Out)
    torch.cuda.synchronize()
    got, xin = ow.cpu().numpy(), xw.cpu().numpy()
    assert np.all(np.isnan(got[:, N:])) and np.all(np.isnan(xin[:, N:]))
    assert np.array_equal(xin[:, :N], U.reshape(n * ks, N))
    return got[:, :N].reshape(n, ks, N)


# ---- 1. parity with the existing operator

@pytest.mark.parametrize("shape", [A, B, C, D], ids=["A", "B", "C", "D"])
def test_every_source_matches_block_op_dev(shape):
    """which = 0, 1, 2 and 1, 2, 3, 4, 5, 7 sources on the shared M2L pass: every source
    <= 1e-12 (relative l2) from block_op_dev of that source on the same handle; the host form
    equals the device form bitwise."""
    a = _handle(shape)
    U = _sources(shape)
    worst = 0.0
    for which in (0, 1, 2):
        ref = _single(shape, which)
        for n in NSRC:
            got = _multi(a, which, U[:n])
            for s in range(n):
                err = _rel(got[s], ref[s])
                worst = max(worst, err)
                assert err <= PARITY, (which, n, s, err)
            if n == 5:
                host = a.block_op_multi(which, U[:n].reshape(n, -1).T)
                assert np.array_equal(host.T.reshape(n, a.ks, a.N), got), which
    print(f"shape {shape}: worst source against block_op_dev {worst:.3e}")


@pytest.mark.parametrize("shape", [E, F, FL], ids=["E", "F-cached", "F-lean"])
def test_the_per_source_route_is_block_op_dev_bit_for_bit(shape):
    """ks > 8 and np = 4 (cached and lean): one block_op_dev per source, so every source's
    bits are that call's; the host form equals the device form bitwise."""
    a = _handle(shape)
    U = _sources(shape)
    for which in (0, 1, 2):
        ref = _single(shape, which)
        for n in NSRC:
            got = _multi(a, which, U[:n])
            assert np.array_equal(got, ref[:n]), (which, n)
            if n == 5:
                host = a.block_op_multi(which, U[:n].reshape(n, -1).T)
                assert np.array_equal(host.T.reshape(n, a.ks, a.N), got), which


# ---- 2. oracle

def _block_ref(o, U, g, ss, which):
    """aniso.m forward / mforward / x - mforward(x) composed from oracle mode applies
    (test_gpu_high_order.py's helper)."""
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


@functools.lru_cache(maxsize=None)
def _oracle_ref(shape, s):
    o = _oracle(shape)
    ss, _ = _coeffs(o.getNodes(), shape[4])
    ref = _block_ref(o, _sources(shape)[s], G, ss, 2)
    ref.setflags(write=False)
    return ref


@pytest.mark.parametrize("shape", [A, B], ids=["A", "B"])
def test_a_four_source_call_matches_the_composed_oracle(shape):
    """Sources 0 and 3 of a 4-source x - mforward(x) against aniso.m's composition of oracle
    mode applies at the same order, <= 1e-10."""
    a = _handle(shape)
    got = _multi(a, 2, _sources(shape)[:4])
    for s in (0, 3):
        err = _rel(got[s], _oracle_ref(shape, s))
        print(f"shape {shape} source {s} of 4: rel err vs composed oracle {err:.3e}")
        assert err <= ORACLE, (s, err)


# ---- 3. property P

@pytest.mark.parametrize("shape", [A, B, C, D], ids=["A", "B", "C", "D"])
def test_a_source_does_not_see_the_call_around_it(shape):
    """Source 2 alone, beside one, among four (first and last) and among seven (in the full
    chunk, in the zero-padded chunk of three, at its end) returns equal bits, for which = 0
    and 2; two identical calls return equal bits; block_op(2) returns the same bits before
    and after a 4-source call, and cache_bytes does not change."""
    a = _handle(shape)
    U = _sources(shape)
    k = 2
    orders = [[2], [5, 2], [2, 0], [2, 0, 1, 3], [6, 4, 3, 2], [0, 1, 2, 3, 4, 5, 6], [6, 5, 4, 3, 2, 1, 0],
              [0, 1, 3, 4, 5, 2, 6], [0, 1, 3, 4, 2, 5, 6], [0, 1, 3, 4, 5, 6, 2], [4, 2, 6]]
    bytes0 = a.cache_bytes()
    before = a.block_op(2, U[0])
    for which in (2, 0):
        first = None
        for order in orders:
            got = _multi(a, which, U[order])[order.index(k)]
            if first is None:
                first = got
            assert np.array_equal(got, first), (which, order)
        assert _rel(first, _single(shape, which)[k]) <= PARITY
    seven = _multi(a, 2, U)
    assert np.array_equal(_multi(a, 2, U), seven)
    _multi(a, 2, U[:4])
    assert np.array_equal(a.block_op(2, U[0]), before)
    assert a.cache_bytes() == bytes0


# ---- 4. solve

def _gaussians(shape, n=4):
    """n charges of ks blocks: Gaussians at n centres, block b scaled by 2^-b: (n, ks, N)."""
    a = _handle(shape)
    xy = a.getNodes()
    cen = [(0.5, 0.5), (0.3, 0.65), (0.7, 0.35), (0.25, 0.25)][:n]
    return np.array([[np.exp(-25.0 * ((xy[:, 0] - cx) ** 2 + (xy[:, 1] - cy) ** 2)) * 0.5 ** b for b in range(a.ks)]
                     for cx, cy in cen])


@functools.lru_cache(maxsize=None)
def _block_solve(shape, s, restart, maxit):
    """block_solve of Gaussian s alone: (steps, x (ks, N), history, relres, rhs (ks, N))."""
    a = _handle(shape)
    rhs = a.block_op(0, _gaussians(shape)[s])
    it, x, hist, relres = a.block_solve(rhs, restart=restart, tol=TOL, maxit=maxit)
    return it, x, hist, relres, rhs


def _clears(hist, it):
    """block_solve's own history (hist[k]: the estimate after step k + 1) clears tol at its
    last step `it` by at least 1 % on both sides (test_gpu_forward_solve_multi.py's rule)."""
    return it > 0 and (it == 1 or hist[it - 2] >= 1.01 * TOL) and hist[it - 1] <= 0.99 * TOL


def _solve(a, Q, X0, restart, maxit, charge=True):
    """block_solve_multi_dev on (n, ks, N) arrays: (iters, relres, hist, X (n, ks, N), calls)."""
    torch = _torch()
    n, ks, N = Q.shape
    Qd = torch.tensor(Q.reshape(n * ks, N), device="cuda")
    Xd = torch.tensor(X0.reshape(n * ks, N), device="cuda")
    iters, relres, hist = a.block_solve_multi_dev(Qd, Xd, restart=restart, tol=TOL, maxit=maxit, rhs_is_charge=charge)
    torch.cuda.synchronize()
    assert torch.equal(Qd, torch.tensor(Q.reshape(n * ks, N), device="cuda"))
    return iters, relres, hist, Xd.cpu().numpy().reshape(n, ks, N), [int(c) for c in a.forward_solve_calls()]


def _expected_calls(groups, restart):
    """The source count of every operator call of a solve whose cycles end at `restart` steps or
    at convergence, and how many of these rows are no Arnoldi step (right-hand sides and explicit
    residuals).  groups: per group a list of (steps, zero right-hand side, zero guess)."""
    calls = []
    for grp in groups:
        calls.append(len(grp))  # forward(charge)
        left = [0 if zero_b else it for it, zero_b, _ in grp]
        first = sum(1 for _, zero_b, zero_x in grp if not zero_b and not zero_x)
        if first:
            calls.append(first)  # the first residuals of the non-zero guesses
        while any(left):
            act = [r for r in left if r > 0]
            for j in range(min(restart, max(act))):
                calls.append(sum(1 for r in act if r > j))
            calls.append(len(act))  # the explicit residuals at the cycle's end
            left = [max(r - restart, 0) for r in left]
    return calls, sum(calls) - sum(it for grp in groups for it, zero_b, _ in grp if not zero_b)


def _check_against_block_solve(a, shape, picks, iters, relres, X, restart, maxit, counts=True):
    """Sources `picks` (index in the call -> Gaussian) against block_solve of each alone: relres
    is the recomputed |b - A x| / |b| (rtol 1e-3); where block_solve converges the source does,
    with its step count under the 1 % rule and its solution to 1e-8; where block_solve runs out
    of cycles the source does too, after the same steps."""
    for c, s in picks.items():
        it, x, hist, rr, rhs = _block_solve(shape, s, restart, maxit)
        res = float(np.linalg.norm(rhs - a.block_op(2, X[c])) / np.linalg.norm(rhs))
        err = _rel(X[c], x)
        n = abs(it)
        print(f"source {c} (Gaussian {s}): {iters[c]} steps (block_solve {it}), relres {relres[c]:.4e}, recomputed "
              f"{res:.4e}, block_solve's {rr:.4e}, x vs block_solve {err:.3e}, its history above "
              f"{hist[n - 2] if n > 1 else 1.0:.4e} below {hist[n - 1]:.4e}")
        assert abs(relres[c] - res) <= 1e-3 * res, (c, relres[c], res)
        if it < 0:
            assert rr > TOL and iters[c] == it and relres[c] > TOL, (c, iters[c], it, relres[c])
            continue
        assert it > 0 and rr <= TOL, (s, it, rr)
        assert iters[c] > 0 and relres[c] <= TOL, (c, iters[c], relres[c])
        if counts and _clears(hist, it):
            assert iters[c] == it, (c, iters[c], it)
        # both residuals <= tol |b| and |A^-1| <= 1 / (1 - sigma_s / sigma_t) = 101 (demo.m): 2e-9
        assert err <= 1e-8, (c, err)


def test_six_sources_against_block_solve_of_each():
    """(32, 1, ks = 3, np = 6), demo.m's coefficients, restart 60, maxit 20, tol 1e-11,
    rhs_is_charge: Gaussians at four centres, a zero column (in the first group, with a guess
    it must overwrite) and a column warm-started at its own converged solution (in the second
    group).  Every non-zero source converges; relres is |b - A x| / |b| recomputed with
    block_op(0) and block_op(2) (rtol 1e-3); the step counts are block_solve's under the 1 %
    rule and the solutions lie <= 1e-8 from its; the zero column returns x = 0, 0 steps,
    relres 0; the warm-started one takes 0 steps; the recorded operator calls are those of
    the lockstep scheme (non-increasing inside a cycle, one residual call behind it, and
    their sum the steps plus the residual and right-hand-side rows); a second call repeats
    every bit, and Gaussian 0 solved alone has the bits it has among the others."""
    a = _handle(A3)
    g = _gaussians(A3)
    ks, N = a.ks, a.N
    restart, maxit = 60, 20
    it0, rr0, h0, x0, calls0 = _solve(a, g[:1], np.zeros((1, ks, N)), restart, maxit)
    assert it0[0] > 0 and rr0[0] <= TOL
    Q = np.array([g[0], g[1], np.zeros((ks, N)), g[2], g[0], g[3]])
    X0 = np.zeros_like(Q)
    X0[2] = 3.0
    X0[4] = x0[0]
    iters, relres, hist, X, calls = _solve(a, Q, X0, restart, maxit)
    print(f"six sources: iters {iters.tolist()}, relres {relres.tolist()}, calls {calls}")
    _check_against_block_solve(a, A3, {0: 0, 1: 1, 3: 2, 5: 3}, iters, relres, X, restart, maxit)
    assert iters[2] == 0 and relres[2] == 0.0 and np.all(X[2] == 0.0) and np.all(hist[2] == 0.0)
    assert iters[4] == 0 and relres[4] <= TOL and np.array_equal(X[4], x0[0]) and relres[4] == rr0[0]
    for c in range(6):
        assert np.all(hist[c, :iters[c]] > 0.0) and np.all(hist[c, iters[c]:] == 0.0), c
    groups = [[(int(iters[c]), c == 2, c != 2) for c in range(4)], [(0, False, False), (int(iters[5]), False, True)]]
    want, other = _expected_calls(groups, restart)
    assert calls == want, (calls, want)
    assert sum(calls) == int(iters.sum()) + other and other >= 6 + 1 + 3 + 1
    iters2, relres2, hist2, X2, calls2 = _solve(a, Q, X0, restart, maxit)
    assert np.array_equal(X2, X) and np.array_equal(iters2, iters) and np.array_equal(relres2, relres)
    assert np.array_equal(hist2, hist) and calls2 == calls
    assert np.array_equal(X[0], x0[0]) and iters[0] == it0[0] and relres[0] == rr0[0]
    assert np.array_equal(hist[0], h0[0])
    assert calls0 == _expected_calls([[(int(it0[0]), False, True)]], restart)[0]


def test_restart_8_matches_block_solve_restart_8():
    """Two Gaussians at restart 8, maxit 20.  GMRES(8) stagnates at this shape -- block_solve
    itself ends after 20 cycles at relative residuals of 0.29 and 0.19 (measured on an MI355X) -- so both
    solvers run every cycle: equal (negative) step counts, relres the recomputed residual, and
    the calls of the lockstep scheme over the 20 cycles.  (The six-source test above has the
    converging restarted case: three of its sources take two cycles of 60.)"""
    a = _handle(A3)
    g = _gaussians(A3, 2)
    restart, maxit = 8, 20
    iters, relres, hist, X, calls = _solve(a, g, np.zeros_like(g), restart, maxit)
    print(f"restart 8: iters {iters.tolist()}, relres {relres.tolist()}")
    _check_against_block_solve(a, A3, {0: 0, 1: 1}, iters, relres, X, restart, maxit)
    assert max(abs(iters)) > restart  # it did restart
    assert calls == _expected_calls([[(abs(int(i)), False, True) for i in iters]], restart)[0], calls


def _two_sources(shape, restart, maxit, counts=True):
    """Two Gaussians against block_solve of each, and again with b = forward(q) given."""
    a = _handle(shape)
    g = _gaussians(shape, 2)
    iters, relres, hist, X, calls = _solve(a, g, np.zeros_like(g), restart, maxit)
    _check_against_block_solve(a, shape, {0: 0, 1: 1}, iters, relres, X, restart, maxit, counts)
    assert calls == _expected_calls([[(abs(int(i)), False, True) for i in iters]], restart)[0], calls
    rhs = np.array([_block_solve(shape, s, restart, maxit)[4] for s in range(2)])
    it_b, rr_b, _, X_b, _ = _solve(a, rhs, np.zeros_like(g), restart, maxit, charge=False)
    for c in range(2):  # b = forward(q) given: the same solve to rounding
        assert (it_b[c] > 0) == (iters[c] > 0) and _rel(X_b[c], X[c]) <= 1e-8, (c, it_b[c], iters[c])
        assert rr_b[c] <= TOL or iters[c] < 0, (c, rr_b[c])
    return iters


def test_two_sources_at_order_8():
    """np = 8 (the shared pass at K padded to 4), restart 60, maxit 20: the checks of the
    six-source test on two Gaussians; both converge."""
    assert np.all(_two_sources(B, 60, 20) > 0)


def test_two_sources_on_a_lean_order_4_handle():
    """np = 4 lean (one block_op_dev per source) on the 16 x 16 grid.
    Restart 60, maxit 20: GMRES(60) stagnates on this grid -- block_solve itself ends after 20
    cycles at a relative residual of 1.3e-5 (default sums) / 1.8e-5 (deterministic sums; measured
    on an MI355X; unrestarted it takes 201 / 202 steps) -- so neither solver converges: both run
    every cycle, with equal step counts, and relres is the recomputed residual.
    Restart 240: both converge; relres and the solutions are checked as in the six-source test.
    The step counts are NOT compared there: block_solve's own count moves from 201 to 202 and
    the last estimates of its history by 20 % between the default and the deterministic sums,
    so at this shape its history is not reproducible to the rule's 1 % under last-bit changes
    of the operator; the multi-source solve takes 199 steps against its 202 (solutions 2.8e-11
    apart, both residuals <= tol)."""
    assert np.all(_two_sources(FL, 60, 20) == -1200)
    assert np.all(_two_sources(FL, 240, 20, counts=False) > 0)


# ---- 5. refusals stay

def test_a_high_order_handle_still_refuses_what_it_refused():
    torch = _torch()
    import aniso_amd

    a = _handle(A)
    N, ks = a.N, a.ks
    _multi(a, 2, _sources(A)[:4])

    def dev(*shape):
        return torch.zeros(*shape, dtype=torch.float64, device="cuda")

    for name, call in [("mapping_batched", lambda: a.mapping_batched(np.ones((N, 2)), 0)),
                       ("gmres", lambda: a.gmres(np.ones(N))),
                       ("block_op_sharded_dev", lambda: a.block_op_sharded_dev(2, dev(ks, N), dev(ks, N)))]:
        with pytest.raises(aniso_amd.AnisoError) as e:
            call()
        assert e.value.code == 3, (name, e.value.code, str(e.value))  # ANISO_ERR_STATE
        assert "high-order" in str(e.value), (name, str(e.value))
