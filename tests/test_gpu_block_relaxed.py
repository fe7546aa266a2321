"""The relaxed-precision block solve of high-order handles (np = 6, 8): the
f32 block operator (block_f32.hip) against the fp64 one of the same handle, and the block
solve as inexact GMRES over it against the fp64 solve.

Operator: the shapes of tests/test_gpu_high_order_block.py that cover every compiled block
count, the padded counts, W and X lists with transposed reads, the 64-lane near form and
trees without an M2L pair.  The bound is the one tests/test_gpu_forward_solve_mixed.py holds
the f32 mode operators to, 3.5e-6 in relative 2-norm on the whole result and on every row
against the norm of the whole reference; forward and mforward must also be at least 1e-10
away, which proves that fp32 ran.

Solve: the three rows of the CPU model of DESIGN.md §3.18.8 -- the tree of case d at ks = 2,
of case a at ks = 4, of case f at ks = 5 -- with rhs = forward(Gaussian rows 0.5^b), restart
60, tol 1e-11, maxit 20."""
import functools

import numpy as np
import pytest

from conftest import gaussian_charge, main_coeffs, rough_coeffs

pytestmark = pytest.mark.gpu

OP_BOUND = 3.5e-6   # tests/test_gpu_forward_solve_mixed.py's bound on an f32 operator
OP_FLOOR = 1e-10    # below this the pass did not run in fp32
G = 0.8
RESTART, TOL, MAXIT = 60, 1e-11, 20

# sz, d, ks, ns, np, maxLevel, coefficients (tests/test_gpu_high_order_block.py's shapes)
CASES = {
    "a": (13, 2, 4, 8, 6, 20, "rough"),   # np 6, K = 4, W and X lists, transposed reads
    "b": (13, 2, 7, 8, 6, 20, "rough"),   # 7 padded to 8, the un-fused subtraction
    "c": (13, 2, 8, 8, 6, 20, "rough"),   # K = 8
    "d": (11, 3, 5, 8, 8, 20, "rough"),   # np 8, K = 5
    "f": (24, 1, 8, 10, 8, 20, "main"),   # uniform depth 2 at np = 8
    "l": (15, 3, 2, 8, 8, 2, "rough"),    # leaves of 121..144 points: the 64-lane near form and its loops
    "m": (12, 2, 3, 8, 6, 1, "rough"),    # no V pair: near field only; 3 padded to 4
    "o": (1, 6, 1, 8, 8, 20, "main"),     # ks = 1 run as 2
}
# the operator cases (case, ks or None for the case's own) and the solve shapes
OP_CASES = [("a", None), ("b", None), ("c", None), ("d", None), ("f", 2), ("l", None), ("m", None), ("o", None)]
SOLVES = [("d", 2), ("a", 4), ("f", 5)]
OPS = pytest.mark.parametrize("case,ks", OP_CASES, ids=[c + ("" if k is None else f"-ks{k}") for c, k in OP_CASES])
SHAPES = pytest.mark.parametrize("case,ks", SOLVES, ids=[f"{c}-ks{k}" for c, k in SOLVES])


def _torch():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def _coeffs(xy, coeffs, seed=7):
    return main_coeffs(xy) if coeffs == "main" else rough_coeffs(xy, seed)


def _new_handle(case, ks=None):
    """A fresh handle of the case's shape (ks blocks) after aniso_cache_block."""
    import aniso_amd

    sz, d, ks0, ns, np_, ml, coeffs = CASES[case]
    a = aniso_amd.Aniso(sz, d, ks0 if ks is None else ks, G, ns, np_, ml)
    a.setCoeff(*_coeffs(a.getNodes(), coeffs))
    a.cache_block()
    return a


@functools.lru_cache(maxsize=None)
def _handle(case, ks=None):
    return _new_handle(case, ks)


@functools.lru_cache(maxsize=None)
def _input(ks, N, seed=5):
    U = np.random.default_rng(seed).uniform(-1.0, 1.0, (ks, N))
    U.setflags(write=False)
    return U


def _dev(torch, X):
    return torch.tensor(np.ascontiguousarray(X), device="cuda")


def _op(a, which, U, f32):
    torch = _torch()
    out = torch.full((a.ks, a.N), float("nan"), dtype=torch.float64, device="cuda")
    (a.block_op_f32_dev if f32 else a.block_op_dev)(which, _dev(torch, U), out)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _distances(got, ref):
    whole = float(np.linalg.norm(got - ref) / np.linalg.norm(ref))
    rows = [float(np.linalg.norm(got[i] - ref[i]) / np.linalg.norm(ref)) for i in range(ref.shape[0])]
    return whole, rows


# ---- the operator

@pytest.mark.parametrize("which", [0, 1, 2])
@OPS
def test_f32_operator_is_close_to_the_fp64_one(case, ks, which):
    """block_op_f32_dev against block_op_dev of the same handle: <= 3.5e-6 whole and per row
    (against the norm of the whole reference), every value finite; forward and mforward are also
    >= 1e-10 away: fp32 ran."""
    a = _handle(case, ks)
    U = _input(a.ks, a.N)
    ref, got = _op(a, which, U, False), _op(a, which, U, True)
    whole, rows = _distances(got, ref)
    print(f"case {case} (np {a.np}, ks {a.ks}, N {a.N}) which {which}: f32 vs fp64 {whole:.3e}, "
          f"rows {' '.join(f'{r:.3e}' for r in rows)}")
    assert np.all(np.isfinite(got)), (case, which)
    assert whole <= OP_BOUND, (case, which, whole)
    assert max(rows) <= OP_BOUND, (case, which, rows)
    if which < 2:
        assert whole >= OP_FLOOR, (case, which, whole)


@OPS
def test_two_identical_f32_calls_return_equal_bits(case, ks):
    a = _handle(case, ks)
    U = _input(a.ks, a.N)
    for which in (0, 2):
        assert np.array_equal(_op(a, which, U, True), _op(a, which, U, True)), (case, which)


def test_strided_rows_return_the_contiguous_bits():
    """Case a with x at row stride N + 7 and out at row stride N + 3, NaN in the gaps of both and
    all over out: the gaps stay NaN, x is unchanged, the result is the contiguous call's."""
    torch = _torch()
    a = _handle("a")
    ks, N = a.ks, a.N
    U = _input(ks, N)
    nan = float("nan")
    for which in (0, 1, 2):
        want = _op(a, which, U, True)
        xw = torch.full((ks, N + 7), nan, dtype=torch.float64, device="cuda")
        xw[:, :N] = _dev(torch, U)
        ow = torch.full((ks, N + 3), nan, dtype=torch.float64, device="cuda")
        a.block_op_f32_dev(which, xw[:, :N], ow[:, :N])
        torch.cuda.synchronize()
        assert torch.isnan(ow[:, N:]).all() and torch.isnan(xw[:, N:]).all(), which
        assert np.array_equal(xw[:, :N].cpu().numpy(), U), which
        assert np.array_equal(ow[:, :N].cpu().numpy(), want), which


@pytest.mark.parametrize("case,ks", [("a", None), ("b", None), ("d", None), ("m", None)])
def test_the_mirrors_and_the_fp64_operator_around_f32_calls(case, ks):
    """On a fresh handle: cache_f32_bytes is 0 before the first f32 call and half of the two
    mirrored E arrays after (cache_bytes()[1] less sigma_t at every point); block_op_dev and
    cache_bytes are what they were before."""
    a = _new_handle(case, ks)
    try:
        U = _input(a.ks, a.N)
        before = [_op(a, which, U, False) for which in (0, 1, 2)]
        bytes0 = a.cache_bytes()
        assert a.cache_f32_bytes() == 0
        expect = (bytes0[1] - 8 * a.N) // 2
        assert expect > 0 and (bytes0[1] - 8 * a.N) % 2 == 0
        for which in (0, 1, 2):
            _op(a, which, U, True)
            assert a.cache_f32_bytes() == expect, (case, which)
        assert a.cache_bytes() == bytes0
        for which in (0, 1, 2):
            assert np.array_equal(_op(a, which, U, False), before[which]), (case, which)
    finally:
        a.close()


# ---- the solve

@functools.lru_cache(maxsize=None)
def _rhs(case, ks):
    a = _handle(case, ks)
    xy = a.getNodes()
    F = np.stack([gaussian_charge(xy) * (0.5 ** b) for b in range(ks)])
    rhs = a.block_op(0, F)
    rhs.setflags(write=False)
    return rhs


def _solve(a, rhs, relax, x0=None):
    """(iters, x, hist, relres, calls) of block_solve_dev (relax = "fp64") or the relaxed entry."""
    torch = _torch()
    b = _dev(torch, rhs)
    x = torch.zeros(a.ks, a.N, dtype=torch.float64, device="cuda") if x0 is None else _dev(torch, x0)
    if relax == "fp64":
        it, hist, rr = a.block_solve_dev(b, x, restart=RESTART, tol=TOL, maxit=MAXIT)
        calls = None
    else:
        it, hist, rr = a.block_solve_relaxed_dev(b, x, restart=RESTART, tol=TOL, maxit=MAXIT, relax=relax)
        calls = a.block_solve_relaxed_calls().copy()
    torch.cuda.synchronize()
    assert np.array_equal(b.cpu().numpy(), rhs)
    return it, x.cpu().numpy(), hist.copy(), rr, calls


@functools.lru_cache(maxsize=None)
def _solved(case, ks, relax):
    return _solve(_handle(case, ks), _rhs(case, ks), relax)


def _cycles_of(calls, what):
    """The passes of a solve from a zero guess, cut at the fp64 passes that follow an f32 one:
    those are cycle-boundary residuals.  The call ends on one, and no cycle holds more Arnoldi
    matvecs than the restart."""
    assert calls.size and calls[-1] == 64, (what, calls)
    run = 0
    for c in calls:
        run = run + 1 if c == 32 else 0
        assert run <= RESTART, (what, calls)


@SHAPES
def test_relax_0_is_the_fp64_solve_bit_for_bit(case, ks):
    """relax = 0 on a fresh handle: iters, relres, hist and x are block_solve_dev's bits, no pass
    is f32 and no mirror is built."""
    a = _new_handle(case, ks)
    try:
        rhs = _rhs(case, ks)
        it0, x0, h0, r0, _ = _solve(a, rhs, "fp64")
        it1, x1, h1, r1, calls = _solve(a, rhs, 0.0)
        print(f"tree {case} ks {ks}: fp64 {it0} steps relres {r0:.3e}; relax 0: {it1} steps, {calls.size} passes")
        assert it0 > 0 and r0 <= TOL
        assert (it1, r1) == (it0, r0) and np.array_equal(h1, h0) and np.array_equal(x1, x0)
        assert calls.size >= it0 and np.all(calls == 64), calls
        assert a.cache_f32_bytes() == 0
    finally:
        a.close()


@SHAPES
def test_relax_1e_5_converges_at_the_fp64_solve_s_cost(case, ks):
    """relax = 1e-5: converged on the explicit fp64 residual; steps <= 1.25 x the fp64 solve's (the
    CPU model needs 1.00-1.03 at the measured operator distance, 1.14 at ten times it); at least
    5 passes in f32, none before the first estimate <= 1e-5, every cycle-boundary pass fp64; the
    solution within 1e-8 of the fp64 solve's (tests/test_gpu_high_order_shard.py's bound for the
    same solve by another route)."""
    relax = 1e-5
    it0, x0, h0, r0, _ = _solved(case, ks, "fp64")
    it, x, hist, rr, calls = _solved(case, ks, relax)
    n32 = int(np.sum(calls == 32))
    dist = float(np.linalg.norm(x - x0) / np.linalg.norm(x0))
    print(f"tree {case} ks {ks} relax {relax:g}: {it} steps ({it0} fp64), relres {rr:.3e} ({r0:.3e}), "
          f"{n32} f32 + {calls.size - n32} fp64 passes, solution {dist:.3e} from the fp64 solve's")
    assert it0 > 0 and r0 <= TOL
    assert it > 0 and rr <= TOL, (it, rr)
    assert it <= 1.25 * it0, (it, it0)
    assert n32 >= 5, calls
    below = np.nonzero(hist <= relax)[0]
    assert below.size, hist
    # from a zero guess pass i of the first cycle is the matvec of V[i]; those up to the step
    # that gave the first estimate <= relax were enqueued on larger estimates
    assert np.all(calls[: below[0] + 1] == 64), (below[0], calls)
    _cycles_of(calls, (case, ks))
    assert dist <= 1e-8, dist


def test_relaxed_solution_solves_the_oracle_operator():
    """The tree of case d, ks = 2: the residual of the relax = 1e-5 solution under the
    ORACLE-composed operator is <= 1e-9 (the bound and the reasoning of
    test_block_solve_on_a_tree_with_w_and_x_lists)."""
    from oracle.oracle_py import Oracle

    case, ks = "d", 2
    sz, d, _, ns, np_, ml, coeffs = CASES[case]
    it, u, _, rr, _ = _solved(case, ks, 1e-5)
    assert it > 0 and rr <= TOL
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
    rhs = _rhs(case, ks)
    res = float(np.linalg.norm(rhs - (u - mf)) / np.linalg.norm(rhs))
    print(f"tree d ks 2 relax 1e-5: relres {rr:.3e}, oracle-composed residual {res:.3e}")
    assert res <= 1e-9, res


@SHAPES
def test_relax_1_runs_every_arnoldi_matvec_in_f32(case, ks):
    """relax = 1: still converged on the explicit fp64 residual within the 20 cycles; the fp64
    passes are exactly the cycle-boundary residuals (one per cycle, the call's last pass among
    them; each step is one f32 pass, plus at most one enqueued ahead per cycle).  Steps printed."""
    it, x, hist, rr, calls = _solved(case, ks, 1.0)
    n64 = int(np.sum(calls == 64))
    n32 = calls.size - n64
    print(f"tree {case} ks {ks} relax 1: {it} steps, relres {rr:.3e}, {n32} f32 passes, {n64} fp64 (cycles)")
    assert it > 0 and rr <= TOL, (it, rr)
    assert calls[0] == 32, calls
    _cycles_of(calls, (case, ks))
    assert 1 <= n64 <= MAXIT and n64 >= -(-it // RESTART), (n64, it)
    assert it <= n32 <= it + n64, (it, n32, n64)
    assert not np.any((calls[1:] == 64) & (calls[:-1] == 64)), calls  # no two residuals in a row


def test_a_nonzero_guess_starts_on_an_fp64_residual():
    """The relax = 1e-5 solution perturbed by 1e-3 (relative) as the guess: converged, and the
    first pass -- the guess's residual -- is fp64."""
    case, ks = "d", 2
    a = _handle(case, ks)
    _, u, _, _, _ = _solved(case, ks, 1e-5)
    guess = u + 1e-3 * np.linalg.norm(u) / np.sqrt(u.size) * np.random.default_rng(3).standard_normal(u.shape)
    it, x, hist, rr, calls = _solve(a, _rhs(case, ks), 1e-5, x0=guess)
    print(f"tree d ks 2 from a guess 1e-3 away: {it} steps, relres {rr:.3e}, passes {calls.tolist()}")
    assert it > 0 and rr <= TOL, (it, rr)
    assert calls[0] == 64 and calls[-1] == 64, calls


def test_a_zero_right_hand_side_returns_zero_without_a_pass():
    a = _handle("d", 2)
    guess = np.ones((a.ks, a.N))
    it, x, hist, rr, calls = _solve(a, np.zeros((a.ks, a.N)), 1e-5, x0=guess)
    assert it == 0 and rr == 0.0 and hist.size == 0 and calls.size == 0, (it, rr, calls)
    assert not x.any()


def test_the_host_entry_returns_the_device_entry_s_bits():
    case, ks = "a", 4
    a = _handle(case, ks)
    it0, x0, h0, r0, calls0 = _solved(case, ks, 1e-5)
    it, x, hist, rr = a.block_solve_relaxed(_rhs(case, ks), restart=RESTART, tol=TOL, maxit=MAXIT, relax=1e-5)
    assert (it, rr) == (it0, r0) and np.array_equal(hist, h0) and np.array_equal(x, x0)
    assert np.array_equal(a.block_solve_relaxed_calls(), calls0)
    # relax=None is the library default 1e6 x tol = 1e-5 here
    it, x, hist, rr = a.block_solve_relaxed(_rhs(case, ks), restart=RESTART, tol=TOL, maxit=MAXIT)
    assert (it, rr) == (it0, r0) and np.array_equal(x, x0)
