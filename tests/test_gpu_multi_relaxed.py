"""Relaxed precision for several sources on high-order handles (np = 6, 8).

Operator: block_op_multi_f32_dev on shapes A-D of tests/test_gpu_block_multi.py.  Every source
must be block_op_f32_dev's of that source BIT FOR BIT (the per-source chain of the f32
multi-source M2L is hm_entry_f32's and every other stage is the same launch), and lie between
OP_FLOOR and OP_BOUND -- the project's bounds for an f32 operator -- from block_op_multi_dev.

Solves: block_solve_multi_relaxed(_dev) on the three trees of tests/test_gpu_block_relaxed.py's
SOLVES and forward_solve_multi_relaxed(_dev) on S1 and S2 of
tests/test_gpu_forward_solve_multi.py.  relax = 0 is the fp64 entry bit for bit; otherwise the
recorded precision of every operator call is replayed from hist under the rule: a step's call
is f32 iff the largest latest estimate among its live columns is <= relax.  (Step 0 of a cycle
after the first uses the cycle's explicit relres, which no entry returns: there the replay
takes the recorded precision and checks the call's column count only.)"""
import functools

import numpy as np
import pytest

from conftest import gaussian_charge, main_coeffs, rough_coeffs

pytestmark = pytest.mark.gpu

OP_BOUND = 3.5e-6   # tests/test_gpu_forward_solve_mixed.py's bound on an f32 operator
OP_FLOOR = 1e-10    # below this the pass did not run in fp32
G = 0.8
NSRC = (1, 2, 3, 4, 5, 7)

# ---- shapes of tests/test_gpu_block_multi.py: sz, d, ks, ns, coefficients, np
OPS = {
    "A": (32, 1, 5, 10, "demo", 6),   # K = 5
    "B": (32, 1, 3, 10, "demo", 8),   # K padded to 4, 64-point leaves
    "C": (19, 3, 2, 8, "rough", 6),   # W and X lists, transposed reads, K = 2
    "D": (16, 1, 8, 10, "main", 6),   # K = 8
}
# ---- trees of tests/test_gpu_block_relaxed.py's SOLVES: sz, d, ks, ns, np, maxLevel, coefficients
TREES = {
    ("d", 2): (11, 3, 2, 8, 8, 20, "rough"),
    ("a", 4): (13, 2, 4, 8, 6, 20, "rough"),
    ("f", 5): (24, 1, 5, 10, 8, 20, "main"),
}
BRESTART, BTOL, BMAXIT = 60, 1e-11, 20
# ---- S1 and S2 of tests/test_gpu_forward_solve_multi.py: np, sz, d, ks, ns, maxLevel, coefficients
FWD = {
    "S1": (6, 32, 1, 3, 10, 20, "main"),
    "S2": (8, 11, 3, 2, 8, 20, "rough"),
}
FRESTART, FTOL, FMAXIT, XTOL = 80, 1e-12, 5, 1e-10


def _torch():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def _rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def _coeffs(xy, coeffs):
    if coeffs == "demo":
        return 20.0 + 0.0 * xy[:, 0], 20.2 + 0.0 * xy[:, 0]
    return main_coeffs(xy) if coeffs == "main" else rough_coeffs(xy, 7)


def _new(sz, d, ks, ns, np_, ml, coeffs):
    import aniso_amd

    a = aniso_amd.Aniso(sz, d, ks, G, ns, np_, ml)
    a.setCoeff(*_coeffs(a.getNodes(), coeffs))
    a.cache_block()
    return a


def _dev(torch, X):
    return torch.tensor(np.ascontiguousarray(X), device="cuda")


# =====================================================================  the operator

@functools.lru_cache(maxsize=None)
def _op_handle(shape):
    sz, d, ks, ns, coeffs, np_ = OPS[shape]
    return _new(sz, d, ks, ns, np_, 20, coeffs)


@functools.lru_cache(maxsize=None)
def _sources(shape):
    a = _op_handle(shape)
    U = np.random.default_rng(100 + a.ks + a.N).uniform(-1.0, 1.0, (7, a.ks, a.N))
    U.setflags(write=False)
    return U


@functools.lru_cache(maxsize=None)
def _single_f32(shape, which):
    """block_op_f32_dev of every source on the same handle: (7, ks, N)."""
    torch = _torch()
    a = _op_handle(shape)
    out = np.zeros_like(_sources(shape))
    for s, U in enumerate(_sources(shape)):
        o = torch.full((a.ks, a.N), float("nan"), dtype=torch.float64, device="cuda")
        a.block_op_f32_dev(which, _dev(torch, U), o)
        torch.cuda.synchronize()
        out[s] = o.cpu().numpy()
    assert np.all(np.isfinite(out))
    out.setflags(write=False)
    return out


def _multi(a, which, U, f32=True):
    """block_op_multi(_f32)_dev of the sources U (n, ks, N) at row stride N + 7 with NaN in the
    gaps of input and output: the gaps stay NaN, the input is as it was.  Returns (n, ks, N)."""
    torch = _torch()
    n, ks, N = U.shape
    xw = torch.full((n * ks, N + 7), float("nan"), dtype=torch.float64, device="cuda")
    xw[:, :N] = _dev(torch, U.reshape(n * ks, N))
    ow = torch.full((n * ks, N + 7), float("nan"), dtype=torch.float64, device="cuda")
    (a.block_op_multi_f32_dev if f32 else a.block_op_multi_dev)(which, xw[:, :N], ow[:, :N])
    torch.cuda.synchronize()
    got, xin = ow.cpu().numpy(), xw.cpu().numpy()
    assert np.all(np.isnan(got[:, N:])) and np.all(np.isnan(xin[:, N:]))
    assert np.array_equal(xin[:, :N], U.reshape(n * ks, N))
    return got[:, :N].reshape(n, ks, N)


@pytest.mark.parametrize("shape", list(OPS))
def test_every_source_is_block_op_f32_dev_bit_for_bit(shape):
    """which = 0, 1, 2 and 1, 2, 3, 4, 5, 7 sources (fours, a remainder of 3 padded to 4, of 2
    and 1): every source's rows are block_op_f32_dev's of that source on the same handle, bit for
    bit; two identical calls return equal bits."""
    a = _op_handle(shape)
    U = _sources(shape)
    for which in (0, 1, 2):
        ref = _single_f32(shape, which)
        for n in NSRC:
            got = _multi(a, which, U[:n])
            for s in range(n):
                assert np.array_equal(got[s], ref[s]), (shape, which, n, s, _rel(got[s], ref[s]))
        assert np.array_equal(_multi(a, which, U[:5]), _multi(a, which, U[:5])), (shape, which)


@pytest.mark.parametrize("shape", ["A", "B"])
def test_a_source_does_not_see_the_call_around_it(shape):
    """Source 0 at positions 0, 2, 5 and 6 among seven, between other sources each time."""
    a = _op_handle(shape)
    U = _sources(shape)
    ref = _single_f32(shape, 2)[0]
    for pos in (0, 2, 5, 6):
        order = [s for s in range(1, 7)]
        order.insert(pos, 0)
        got = _multi(a, 2, U[order])
        assert np.array_equal(got[pos], ref), (shape, pos)


@pytest.mark.parametrize("shape", list(OPS))
def test_the_f32_operator_is_close_to_the_fp64_one_and_leaves_it_alone(shape):
    """7 and 3 sources against block_op_multi_dev: every source <= 3.5e-6 in relative 2-norm,
    whole and per row against the whole source's norm, and (which < 2) >= 1e-10: fp32 ran.  The
    fp64 operator returns its earlier bits after the f32 calls."""
    a = _op_handle(shape)
    U = _sources(shape)
    for which in (0, 1, 2):
        ref = _multi(a, which, U, f32=False)
        for n in (7, 3):
            got = _multi(a, which, U[:n])
            for s in range(n):
                whole = _rel(got[s], ref[s])
                rows = [float(np.linalg.norm(got[s, i] - ref[s, i]) / np.linalg.norm(ref[s])) for i in range(a.ks)]
                if n == 7:
                    print(f"shape {shape} which {which} source {s}: f32 vs fp64 {whole:.3e}, worst row {max(rows):.3e}")
                assert whole <= OP_BOUND and max(rows) <= OP_BOUND, (shape, which, n, s, whole, rows)
                if which < 2:
                    assert whole >= OP_FLOOR, (shape, which, n, s, whole)
        assert np.array_equal(_multi(a, which, U, f32=False), ref), (shape, which)


# =====================================================================  the rule, replayed

def _replay(calls, iters, hist, zero, group, restart, tol, maxit, relax, rhs_call):
    """Walk the recorded {precision, columns} of a solve from zero guesses through the lockstep
    loop, group by group, and assert every call against the rule.  zero: the columns whose
    right-hand side is 0 (they take no step)."""
    calls = [tuple(int(v) for v in c) for c in calls]
    k = 0
    n = len(iters)
    for g0 in range(0, n, group):
        cols = list(range(g0, min(n, g0 + group)))
        if rhs_call:
            assert calls[k] == (64, len(cols)), (k, calls[k])
            k += 1
        total = {c: abs(int(iters[c])) for c in cols}
        used = {c: 0 for c in cols}
        est = {c: 1.0 for c in cols}  # x = 0: r = b, the explicit relres of the first cycle is 1
        for cyc in range(maxit):
            act = [c for c in cols if c not in zero and used[c] < total[c]]
            if not act:
                break
            frozen = set()
            for j in range(restart):
                live = [c for c in act if c not in frozen]
                if not live:
                    break
                prec, ncols = calls[k]
                assert ncols == len(live), (k, calls[k], live)
                if est[live[0]] is None:  # step 0 of a later cycle: the explicit relres is not returned
                    assert prec == 64 or relax > 0.0, (k, calls[k])
                else:
                    low = relax > 0.0 and max(est[c] for c in live) <= relax
                    assert prec == (32 if low else 64), (k, calls[k], cyc, j, [est[c] for c in live], relax)
                k += 1
                for c in live:
                    e = float(hist[c, used[c]])
                    used[c] += 1
                    est[c] = e
                    if e <= tol or used[c] == total[c]:
                        frozen.add(c)
            assert calls[k] == (64, len(act)), (k, calls[k], act)  # the cycle's end: an fp64 residual
            k += 1
            for c in act:
                est[c] = None
        for c in cols:
            assert used[c] == total[c], (c, used[c], total[c])
    assert k == len(calls), (k, len(calls))


# =====================================================================  the block solve

@functools.lru_cache(maxsize=None)
def _tree(key):
    return _new(*TREES[key])


@functools.lru_cache(maxsize=None)
def _charges(key):
    """Five sources: Gaussian rows 0.5^b at four centres, and an all-zero source in the middle."""
    a = _tree(key)
    xy = a.getNodes()
    Q = np.zeros((5, a.ks, a.N))
    for s, (cx, cy) in zip((0, 1, 3, 4), ((0.5, 0.5), (0.3, 0.6), (0.7, 0.35), (0.45, 0.25))):
        gs = np.exp(-25 * ((xy[:, 0] - cx) ** 2 + (xy[:, 1] - cy) ** 2))
        for b in range(a.ks):
            Q[s, b] = gs * 0.5 ** b
    assert np.array_equal(Q[0, 0], gaussian_charge(xy))
    Q.setflags(write=False)
    return Q


def _bsolve(a, Q, relax, restart=BRESTART, maxit=BMAXIT, x0=None, charge=True):
    """(iters, relres, hist, X, calls, counts) of block_solve_multi_dev (relax = "fp64") or the
    relaxed entry; the zero source starts from a guess of 3 that must be overwritten."""
    torch = _torch()
    n, ks, N = Q.shape
    qd = _dev(torch, Q.reshape(n * ks, N))
    if x0 is None:
        x0 = np.zeros((n, ks, N))
        x0[[s for s in range(n) if not Q[s].any()]] = 3.0
    xd = _dev(torch, x0.reshape(n * ks, N))
    if relax == "fp64":
        it, rr, hist = a.block_solve_multi_dev(qd, xd, restart=restart, tol=BTOL, maxit=maxit, rhs_is_charge=charge)
        calls = None
    else:
        it, rr, hist = a.block_solve_multi_relaxed_dev(qd, xd, restart=restart, tol=BTOL, maxit=maxit, relax=relax,
                                                       rhs_is_charge=charge)
        calls = a.solve_multi_relaxed_calls().copy()
    counts = np.array(a.forward_solve_calls())
    torch.cuda.synchronize()
    assert np.array_equal(qd.cpu().numpy(), Q.reshape(n * ks, N))
    return it.copy(), rr.copy(), hist.copy(), xd.cpu().numpy().reshape(n, ks, N), calls, counts


@functools.lru_cache(maxsize=None)
def _bsolved(key, relax):
    return _bsolve(_tree(key), _charges(key), relax)


@functools.lru_cache(maxsize=None)
def _bresiduals(key, relax):
    """|b - A x| / |b| of every nonzero source of _bsolved(key, relax) through the fp64 entries."""
    a, Q = _tree(key), _charges(key)
    X = _bsolved(key, relax)[3]
    b = _multi(a, 0, Q, f32=False)
    w = _multi(a, 2, X, f32=False)
    return {s: float(np.linalg.norm(b[s] - w[s]) / np.linalg.norm(b[s])) for s in (0, 1, 3, 4)}


BSHAPES = pytest.mark.parametrize("key", list(TREES), ids=[f"{c}-ks{k}" for c, k in TREES])


@BSHAPES
def test_block_relax_0_is_the_fp64_solve_bit_for_bit(key):
    a = _new(*TREES[key])
    try:
        Q = _charges(key)
        it0, rr0, h0, x0, _, n0 = _bsolve(a, Q, "fp64")
        it1, rr1, h1, x1, calls, n1 = _bsolve(a, Q, 0.0)
        print(f"tree {key}: fp64 steps {it0.tolist()}, relres {rr0}")
        assert np.all(it0[[0, 1, 3, 4]] > 0) and np.all(rr0 <= BTOL)
        assert np.array_equal(it1, it0) and np.array_equal(rr1, rr0) and np.array_equal(h1, h0)
        assert np.array_equal(x1, x0)
        assert np.all(calls[:, 0] == 64) and np.array_equal(calls[:, 1], n0) and np.array_equal(n1, n0)
        assert a.cache_f32_bytes() == 0
    finally:
        a.close()


@BSHAPES
def test_block_relax_1e_5_converges_under_the_replayed_rule(key):
    """relax = 1e-5: every source converged on the explicit fp64 residual, which the fp64
    entries reproduce to 5 digits; steps <= 1.25 x the fp64 multi solve's per source (the
    allowance of tests/test_gpu_block_relaxed.py from the CPU model: under the group rule a
    source runs in f32 at no step where its own rule would not); solutions within 1e-8; at least
    one f32 call; the recorded precisions are the rule's; the column counts are
    forward_solve_calls'."""
    relax = 1e-5
    it0, rr0, _, x0, _, _ = _bsolved(key, "fp64")
    it, rr, hist, x, calls, counts = _bsolved(key, relax)
    res = _bresiduals(key, relax)
    n32 = int(np.sum(calls[:, 0] == 32))
    print(f"tree {key} relax {relax:g}: steps {it.tolist()} (fp64 {it0.tolist()}), relres {rr}, "
          f"{n32} f32 + {len(calls) - n32} fp64 calls")
    for s in (0, 1, 3, 4):
        dist = _rel(x[s], x0[s])
        print(f"  source {s}: recomputed residual {res[s]:.6e} (reported {rr[s]:.6e}), solution {dist:.3e} from fp64's")
        assert it[s] > 0 and rr[s] <= BTOL, (s, it[s], rr[s])
        assert abs(res[s] - rr[s]) <= 1e-5 * rr[s], (s, res[s], rr[s])
        assert it[s] <= 1.25 * it0[s], (s, it[s], it0[s])
        assert dist <= 1e-8, (s, dist)
    assert it[2] == 0 and rr[2] == 0.0 and not x[2].any() and not hist[2].any()
    assert n32 >= 1, calls
    assert np.array_equal(calls[:, 1], counts)
    _replay(calls, it, hist, {2}, 4, BRESTART, BTOL, BMAXIT, relax, True)


@BSHAPES
def test_block_relax_1_runs_every_arnoldi_call_in_f32(key):
    it, rr, hist, x, calls, counts = _bsolved(key, 1.0)
    print(f"tree {key} relax 1: steps {it.tolist()}, relres {rr}, calls {calls[:, 0].tolist()}")
    assert np.all(it[[0, 1, 3, 4]] > 0) and np.all(rr <= BTOL), (it, rr)
    _replay(calls, it, hist, {2}, 4, BRESTART, BTOL, BMAXIT, 1.0, True)
    # the fp64 calls are forward(charge) of each group and one residual per cycle: none between
    # two Arnoldi steps of a cycle, which the replay has checked call by call; count them too
    arnoldi = int(np.sum(np.abs(it)))
    assert int(np.sum(calls[calls[:, 0] == 32, 1])) == arnoldi, (calls, it)


def test_block_warm_start_not_converged_host_entry_and_repeat():
    """Tree d, ks 2.  A warm start from the solution: 0 steps after one fp64 residual call.
    restart 8, maxit 2: negative iters and the explicit fp64 relres.  The host entry returns the
    device entry's bits, and a second device call repeats every bit."""
    key = ("d", 2)
    a, Q = _tree(key), _charges(key)
    it0, rr0, h0, x0, calls0, _ = _bsolved(key, 1e-5)
    it, rr, hist, x, calls, _ = _bsolve(a, Q, 1e-5, x0=x0)
    assert np.all(it == 0) and np.all(rr <= BTOL) and np.array_equal(x[[0, 1, 3, 4]], x0[[0, 1, 3, 4]]), (it, rr)
    # per group: forward(charge) of its sources, then ONE fp64 residual call on the nonzero ones
    assert calls.tolist() == [[64, 4], [64, 3], [64, 1], [64, 1]], calls
    it, rr, hist, x, calls, _ = _bsolve(a, Q, 1e-5, restart=8, maxit=2)
    b, w = _multi(a, 0, Q, f32=False), _multi(a, 2, x, f32=False)
    for s in (0, 1, 3, 4):
        res = float(np.linalg.norm(b[s] - w[s]) / np.linalg.norm(b[s]))
        print(f"restart 8 x 2, source {s}: iters {it[s]}, relres {rr[s]:.6e}, recomputed {res:.6e}")
        assert it[s] == -16 and rr[s] > BTOL, (s, it[s], rr[s])
        assert abs(res - rr[s]) <= 1e-5 * rr[s], (s, res, rr[s])
    assert it[2] == 0 and rr[2] == 0.0
    _replay(calls, it, hist, {2}, 4, 8, BTOL, 2, 1e-5, True)
    X, ith, rrh = a.block_solve_multi_relaxed(Q.reshape(5, -1).T, restart=BRESTART, tol=BTOL, maxit=BMAXIT, relax=1e-5)
    assert np.array_equal(ith, it0) and np.array_equal(rrh, rr0)
    assert np.array_equal(X.T.reshape(x0.shape), x0)
    assert np.array_equal(a.solve_multi_relaxed_calls(), calls0)
    again = _bsolve(a, Q, 1e-5)
    for u, v in zip(again, _bsolved(key, 1e-5)):
        assert np.array_equal(u, v)
    # relax < 0 is the default 1e6 x tol = 1e-5 here
    it, rr, hist, x, calls, _ = _bsolve(a, Q, -1.0)
    assert np.array_equal(it, it0) and np.array_equal(x, x0) and np.array_equal(calls, calls0)


def test_block_relaxed_solution_solves_the_oracle_operator():
    """Tree d, ks 2, source 1 of the relax = 1e-5 solve: its residual under the ORACLE-composed
    operator is <= 1e-9 (tests/test_gpu_block_relaxed.py's bound and reasoning)."""
    from oracle.oracle_py import Oracle

    key, s = ("d", 2), 1
    sz, d, ks, ns, np_, ml, coeffs = TREES[key]
    a = _tree(key)
    it, rr, _, X, _, _ = _bsolved(key, 1e-5)
    assert it[s] > 0 and rr[s] <= BTOL
    u = X[s]
    o = Oracle(sz, d, ks, G, ns, np_, ml)
    ss, st = _coeffs(o.getNodes(), coeffs)
    o.setCoeff(ss, st)
    for m in range(2 * ks - 1):
        o.cache(m)
    mf = np.zeros_like(u)
    for i in range(ks):
        for j in range(-(ks - 1), ks):
            w = (G ** abs(j) - G ** ks) / (1 - G ** ks)
            mf[i] += w * o.mapping(u[abs(j)] * ss, abs(i - j))
    rhs = a.block_op(0, _charges(key)[s])
    res = float(np.linalg.norm(rhs - (u - mf)) / np.linalg.norm(rhs))
    print(f"tree d ks 2 source {s} relax 1e-5: relres {rr[s]:.3e}, oracle-composed residual {res:.3e}")
    assert res <= 1e-9, res


# =====================================================================  the forward solve

@functools.lru_cache(maxsize=None)
def _fwd_handle(shape):
    np_, sz, d, ks, ns, ml, coeffs = FWD[shape]
    return _new(sz, d, ks, ns, np_, ml, coeffs)


@functools.lru_cache(maxsize=None)
def _columns(shape):
    """The six "mixed" columns of tests/test_gpu_forward_solve_multi.py, repeated at scales
    0.5^r to 16 columns."""
    xy = _fwd_handle(shape).getNodes()
    N = xy.shape[0]
    rng = np.random.default_rng(11 + N)
    x, y = xy[:, 0], xy[:, 1]
    six = np.array([gaussian_charge(xy), rng.uniform(-1.0, 1.0, N), np.exp(-200.0 * ((x - 0.2) ** 2 + (y - 0.7) ** 2)),
                    np.ones(N), 1e-3 * rng.uniform(-1.0, 1.0, N), (x > 0.5).astype(np.float64)])
    Q = np.array([six[j % 6] * 0.5 ** (j // 6) for j in range(16)])
    Q.setflags(write=False)
    return Q


def _fsolve(a, Q, relax, source=True, x0=None):
    torch = _torch()
    qd = _dev(torch, Q)
    xd = torch.zeros_like(qd) if x0 is None else _dev(torch, x0)
    if relax == "fp64":
        it, rr, hist = a.forward_solve_multi_dev(qd, xd, restart=FRESTART, tol=FTOL, maxit=FMAXIT, rhs_is_source=source)
        calls = None
    else:
        it, rr, hist = a.forward_solve_multi_relaxed_dev(qd, xd, restart=FRESTART, tol=FTOL, maxit=FMAXIT, relax=relax,
                                                         rhs_is_source=source)
        calls = a.solve_multi_relaxed_calls().copy()
    counts = np.array(a.forward_solve_calls())
    torch.cuda.synchronize()
    return it.copy(), rr.copy(), hist.copy(), xd.cpu().numpy(), calls, counts


@pytest.mark.parametrize("wide,n", [(False, 1), (False, 5), (False, 8), (False, 11), (True, 16)],
                         ids=["1", "5", "8", "11", "wide16"])
@pytest.mark.parametrize("shape", list(FWD))
def test_forward_relaxed_against_the_fp64_solve(shape, wide, n):
    """relax = 0: forward_solve_multi_dev's bits, every call fp64.  The default relax (1e6 x tol
    = 1e-6): converged, steps <= 1.25 x the fp64 count per column, solutions within XTOL, at least
    one f32 call, the rule replayed (groups of 8, or 16 with the wide setting on), a bitwise
    repeat."""
    a = _fwd_handle(shape)
    Q = _columns(shape)[:n]
    group = 16 if wide else 8
    a.set_wide(wide)
    try:
        it0, rr0, h0, x0, _, n0 = _fsolve(a, Q, "fp64")
        it1, rr1, h1, x1, calls, n1 = _fsolve(a, Q, 0.0)
        assert np.all(it0 > 0) and np.all(rr0 <= FTOL), (it0, rr0)
        assert np.array_equal(it1, it0) and np.array_equal(rr1, rr0) and np.array_equal(h1, h0)
        assert np.array_equal(x1, x0)
        assert np.all(calls[:, 0] == 64) and np.array_equal(calls[:, 1], n0) and np.array_equal(n1, n0)
        it, rr, hist, x, calls, counts = _fsolve(a, Q, -1.0)
        n32 = int(np.sum(calls[:, 0] == 32))
        print(f"{shape} {n} columns{' wide' if wide else ''}: steps {it.tolist()} (fp64 {it0.tolist()}), "
              f"{n32} f32 + {len(calls) - n32} fp64 calls, worst relres {rr.max():.3e}")
        assert np.all(it > 0) and np.all(rr <= FTOL), (it, rr)
        for c in range(n):
            assert it[c] <= 1.25 * it0[c], (c, it[c], it0[c])
            assert _rel(x[c], x0[c]) <= XTOL, (c, _rel(x[c], x0[c]))
        assert n32 >= 1, calls
        assert np.array_equal(calls[:, 1], counts)
        _replay(calls, it, hist, set(), group, FRESTART, FTOL, FMAXIT, 1e6 * FTOL, False)
        again = _fsolve(a, Q, -1.0)
        for u, v in zip(again, (it, rr, hist, x, calls, counts)):
            assert np.array_equal(u, v)
    finally:
        a.set_wide(False)


def test_forward_zero_column_given_right_hand_side_and_host_entry():
    """S2: an all-zero column in the middle returns x = 0, 0 steps and relres 0; a given
    right-hand side (rhs_is_source = 0) takes the same steps to the same solution (the call that
    forms the right-hand sides is not an operator call of the solve: neither list records it);
    the host entry returns the device entry's bits."""
    torch = _torch()
    a = _fwd_handle("S2")
    Q = _columns("S2")[:5].copy()
    Q[2] = 0.0
    x0 = np.zeros_like(Q)
    x0[2] = 3.0
    it, rr, hist, x, calls, _ = _fsolve(a, Q, 1e-6, x0=x0)
    assert it[2] == 0 and rr[2] == 0.0 and not x[2].any() and not hist[2].any()
    assert np.all(it[[0, 1, 3, 4]] > 0) and np.all(rr <= FTOL)
    _replay(calls, it, hist, {2}, 8, FRESTART, FTOL, FMAXIT, 1e-6, False)
    B = torch.zeros(5, a.N, dtype=torch.float64, device="cuda")
    a.mapping_multi_dev(_dev(torch, Q), 0, B)
    torch.cuda.synchronize()
    itb, rrb, histb, xb, callsb, _ = _fsolve(a, B.cpu().numpy(), 1e-6, source=False, x0=x0)
    assert np.array_equal(itb, it) and np.array_equal(xb, x) and np.array_equal(histb, hist)
    assert np.array_equal(callsb, calls)
    _replay(callsb, itb, histb, {2}, 8, FRESTART, FTOL, FMAXIT, 1e-6, False)
    X, ith, rrh = a.forward_solve_multi_relaxed(Q.T, restart=FRESTART, tol=FTOL, maxit=FMAXIT, relax=1e-6)
    assert np.array_equal(ith, it) and np.array_equal(rrh, rr) and np.array_equal(X.T, x)
