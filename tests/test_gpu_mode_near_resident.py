"""The resident near field of a high-order handle on the GPU: after
cache_mode_near(id) the fp64 mode applies run the MFMA near field of mode_near_resident.hip on
the stored near factor blocks, and with cache_mode's M2L blocks resident too a 16-column chunk
runs one near launch.  Against the CPU oracle at the same order and against the same call with
nothing resident (the mode kernels), column by column; the launches each state takes; bits; the
forward form and the multi-source solve; and what the blocks' life looks like.

The handles, the columns, the oracle's answers and the mode kernels' answers of the shapes
test_gpu_mode_resident.py uses are that module's (computed once for both files); every test
here frees what it made resident."""
import functools

import numpy as np
import pytest

import test_gpu_mode_resident as base
from test_gpu_mode_resident import (_apply, _coeffs, _columns, _handle, _new_handle, _oracle_columns, _oracle_mode,
                                    _rel, _rows, _sources, _torch)

pytestmark = pytest.mark.gpu

TOL = 1e-10     # the suite's oracle-parity bound
ROUTE = 1e-12   # routes that differ by summation order only

# np, sz, d, ks, ns, maxLevel, coefficients: what each exercises in k_near_resident
SHAPES = [
    (6, 32, 1, 3, 10, 20, "demo"),   # 16-point leaves: exactly one tile per leaf, S a multiple of 16
    (6, 19, 3, 2, 8, 20, "rough"),   # W and X lists, leaves of 9..36 points: ragged quads, partial tiles, ragged S
    (6, 20, 2, 2, 8, 2, "rough"),    # 100-point leaves: 7 tiles per leaf, the tile loop
    (8, 11, 3, 2, 8, 20, "rough"),   # np = 8 with W and X lists, leaves of 12..64 points
    (8, 32, 1, 3, 10, 20, "demo"),   # 64-point leaves: four full tiles
    (6, 12, 2, 3, 6, 1, "rough"),    # four 144-point leaves and no V pair: the near field is the whole sum
    (6, 8, 2, 2, 6, 0, "rough"),     # the root as one 256-point leaf whose only source is itself
]
DEMO = [SHAPES[0], SHAPES[4]]
_ID = lambda s: f"np{s[0]}sz{s[1]}d{s[2]}ks{s[3]}ml{s[5]}" if isinstance(s, tuple) else str(s)  # noqa: E731


def _free(a):
    a.cache_mode_near_free()
    a.cache_mode_free()


@functools.lru_cache(maxsize=None)
def _plain_columns(shape, m):
    """mapping_multi_dev of all 19 columns with nothing resident: the mode kernels."""
    _handle(shape).cache_mode_near_free()
    return base._plain_columns(shape, m)


def _near(a):
    c = a.mode_near_calls()
    return c[:, 0].tolist(), c[:, 1].tolist()


def _stored(cols):
    """The flags of near launches of these widths on a near-resident mode: the stored blocks
    serve the full 8-column chunk and the 16-column launch; a padded chunk of 2, 4 or 5 columns
    stays on k_near_mode, which is no slower there."""
    return [1 if c in (8, 16) else 0 for c in cols]


# ---- 1. parity

@pytest.mark.parametrize("nrhs", [1, 3, 8, 11, 16, 19])
@pytest.mark.parametrize("shape", SHAPES, ids=_ID)
def test_every_column_matches_the_oracle_and_the_mode_kernels(shape, nrhs):
    """Modes 0 (the sigma_t diagonal), 1 (odd: the sign of dx) and 2 ks - 2; nrhs = 1, 3 (padded
    narrow chunks), 8, 11 = 8 + 3, 16 = 8 + 8 and 19 = 16 + 3; near blocks alone and near + M2L
    blocks.  Rows of stride N + 7 in and N + 3 out with NaN in the gaps.  Every column: relative
    l2 <= 1e-10 against the oracle at the same order and <= 1e-12 against the same call with
    nothing resident (measured: see DESIGN.md §3.18.7).  The gaps and x are left alone."""
    torch = _torch()
    a = _handle(shape)
    N, ks = a.N, shape[3]
    cols = _columns(N)[:nrhs]
    for m in (0, 1, 2 * ks - 2):
        plain = _plain_columns(shape, m)
        want = _oracle_columns(shape, m)
        for state in ("near", "near + M2L"):
            _free(a)
            a.cache_mode_near(m)
            if state != "near":
                a.cache_mode(m)
            try:
                X = _rows(torch, cols, 7)
                Out = _rows(torch, np.zeros((nrhs, N)), 3)
                a.mapping_multi_dev(X, m, Out)
                torch.cuda.synchronize()
                launches, flags = _near(a)
            finally:
                _free(a)
            assert launches and flags == _stored(launches), (m, state, launches, flags)
            got, x = Out.cpu().numpy(), X.cpu().numpy()
            assert np.all(np.isnan(got[:, N:])), (m, state)
            assert np.all(np.isnan(x[:, N:])) and np.array_equal(x[:, :N], cols), (m, state)
            worst = [0.0, 0.0]
            for j in range(nrhs):
                eo = _rel(got[j, :N], want[j])
                ep = _rel(got[j, :N], plain[j])
                worst = [max(worst[0], eo), max(worst[1], ep)]
            print(f"{_ID(shape)} mode {m} nrhs {nrhs} {state}: worst column vs oracle {worst[0]:.3e}, "
                  f"vs the mode kernels {worst[1]:.3e}")
            assert worst[0] <= TOL, (m, state, worst)
            assert worst[1] <= ROUTE, (m, state, worst)


# ---- 2. the route

NARROW = {8: [8], 9: [8, 2], 11: [8, 4], 16: [8, 8], 19: [8, 8, 4]}
WIDE = {8: [8], 9: [16], 11: [16], 16: [16], 19: [16, 4]}


@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[4]], ids=_ID)
def test_the_near_launches_of_every_state(shape):
    torch = _torch()
    a = _handle(shape)
    _free(a)
    cols = _columns(a.N)
    m = 1

    def check(apply_want, near_want, flag):
        for n in NARROW:
            _apply(torch, a, cols[:n], m)
            assert a.mode_apply_calls().tolist() == apply_want[n], (n, a.mode_apply_calls())
            nc, fl = _near(a)
            assert nc == near_want[n] and fl == ([0] * len(nc) if not flag else _stored(nc)), (n, nc, fl)

    try:
        check(NARROW, NARROW, 0)             # nothing resident
        nothing = _apply(torch, a, cols, m)
        a.cache_mode_near(m)
        check(NARROW, NARROW, 1)             # near only: every full chunk on the stored blocks
        _apply(torch, a, cols[:11], 0)       # another mode has no near blocks
        assert _near(a) == ([8, 4], [0, 0])
        a.cache_mode_near_free(m)
        a.cache_mode(m)
        check(WIDE, NARROW, 0)               # M2L only: a wide chunk's near field is two launches
        a.cache_mode_near(m)
        check(WIDE, WIDE, 1)                 # both: one near launch per chunk
        # the f32 entry ignores the near blocks
        Out = torch.zeros(11, a.N, dtype=torch.float64, device="cuda")
        a.mapping_multi_f32_dev(torch.tensor(cols[:11], device="cuda"), m, Out)
        torch.cuda.synchronize()
        assert _near(a) == ([8, 4], [0, 0])
        a.cache_mode_near_free(m)
        check(WIDE, NARROW, 0)               # freed: the mode kernels again
        assert a.cache_mode_bytes() > 0      # (the M2L blocks were left)
        a.cache_mode_free(m)
        check(NARROW, NARROW, 0)
        assert np.array_equal(_apply(torch, a, cols, m), nothing)
    finally:
        _free(a)


# ---- 3. bits

@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[2], SHAPES[3]], ids=_ID)
def test_repeats_are_bitwise_equal_and_columns_do_not_meet(shape):
    """Two identical calls: equal bits, with the near blocks alone and with both.  The host entry
    equals the device entry.  With both and 16 columns: every column but one replaced with other
    data leaves the kept column's bits unchanged (one in each half).  block_op(2) returns the
    same bits before and after cache_mode_near and an 8-column call."""
    torch = _torch()
    a = _handle(shape)
    _free(a)
    ks = shape[3]
    cols = _columns(a.N)
    other = np.random.default_rng(99).uniform(-3.0, 3.0, cols.shape)
    U = np.random.default_rng(5).uniform(-1.0, 1.0, (ks, a.N))
    block = a.block_op(2, U)
    try:
        for m in (0, 1):
            a.cache_mode_near(m)
            first = _apply(torch, a, cols, m)
            assert a.mode_apply_calls().tolist() == [8, 8, 4]
            assert np.array_equal(first, _apply(torch, a, cols, m)), m
            assert np.array_equal(a.mapping_multi(cols.T, m).T, first), m
            _apply(torch, a, cols[:8], m)
            assert np.array_equal(a.block_op(2, U), block), m
            a.cache_mode(m)
            first = _apply(torch, a, cols[:16], m)
            assert _near(a) == ([16], [1])
            assert np.array_equal(first, _apply(torch, a, cols[:16], m)), m
            for keep in (3, 12):
                mixed = other[:16].copy()
                mixed[keep] = cols[keep]
                assert np.array_equal(_apply(torch, a, mixed, m)[keep], first[keep]), (m, keep)
            dev = _apply(torch, a, cols, m)
            assert a.mode_apply_calls().tolist() == [16, 4]
            assert np.array_equal(a.mapping_multi(cols.T, m).T, dev), m
            _free(a)
    finally:
        _free(a)


# ---- 4. the forward form and the solve

@pytest.mark.parametrize("shape", DEMO, ids=_ID)
def test_forward_form_and_solve_on_near_resident_mode_0(shape):
    """forward_multi_dev with mode 0's near and M2L blocks resident within 1e-12 of the call with
    nothing resident (11 columns: a wide chunk with a padded half); forward_solve_multi_dev with
    the 5 Gaussian sources of test_gpu_mode_resident.py (their step counts are well defined: see
    there), restart 80, tol 1e-12: relres <= tol in every column, the step counts of the plain
    route's solve, the solutions within 1e-10 of its solutions."""
    torch = _torch()
    a = _handle(shape)
    _free(a)
    N = a.N
    X11 = torch.tensor(_columns(N)[:11], device="cuda")
    Q = torch.tensor(_sources(shape), device="cuda")

    def forward(X):
        out = torch.zeros(X.shape[0], N, dtype=torch.float64, device="cuda")
        a.forward_multi_dev(X, out)
        torch.cuda.synchronize()
        return out.cpu().numpy()

    def solve():
        U = torch.zeros(5, N, dtype=torch.float64, device="cuda")
        iters, relres, _ = a.forward_solve_multi_dev(Q, U, restart=80, tol=1e-12)
        torch.cuda.synchronize()
        return U.cpu().numpy(), iters, relres

    plain = forward(X11)
    U0, iters0, _ = solve()
    a.cache_mode_near(0)
    a.cache_mode(0)
    try:
        res = forward(X11)
        assert a.mode_apply_calls().tolist() == [16] and _near(a) == ([16], [1])
        U, iters, relres = solve()
    finally:
        _free(a)
    worst = max(_rel(res[j], plain[j]) for j in range(11))
    print(f"{_ID(shape)} forward form, near + M2L blocks vs the mode kernels: worst column {worst:.3e}")
    assert worst <= ROUTE, worst
    assert np.all(iters > 0) and np.all(relres <= 1e-12), (iters, relres)
    assert np.array_equal(iters, iters0), (iters, iters0)
    for j in range(5):
        e = _rel(U[j], U0[j])
        print(f"{_ID(shape)} source {j}: {iters[j]} steps, relres {relres[j]:.3e}, solution vs the plain route's {e:.3e}")
        assert e <= TOL, (j, e)


# ---- 5. lifecycle

@pytest.mark.parametrize("shape", DEMO, ids=_ID)
def test_the_life_of_the_near_blocks(shape):
    torch = _torch()
    a = _new_handle(shape)
    N = a.N
    cols = _columns(N)[:11]
    before, f32 = a.cache_bytes(), a.cache_f32_bytes()

    def others_unchanged():
        assert a.cache_bytes() == before and a.cache_f32_bytes() == f32

    assert a.cache_mode_near_bytes() == 0
    a.cache_mode_near(0)
    one = a.cache_mode_near_bytes()
    assert one > 0 and a.cache_mode_bytes() == 0
    a.cache_mode_near(0)
    assert a.cache_mode_near_bytes() == one
    a.cache_mode_near(1)
    assert a.cache_mode_near_bytes() == 2 * one
    others_unchanged()
    # the M2L blocks come and go without touching the near blocks, and the reverse
    a.cache_mode(1)
    m2l = a.cache_mode_bytes()
    assert m2l > 0 and a.cache_mode_near_bytes() == 2 * one
    a.cache_mode_near_free(0)
    assert a.cache_mode_near_bytes() == one and a.cache_mode_bytes() == m2l
    a.cache_mode_free()
    assert a.cache_mode_bytes() == 0 and a.cache_mode_near_bytes() == one
    a.cache_mode(0)
    a.cache_mode_near_free(-1)
    assert a.cache_mode_near_bytes() == 0 and a.cache_mode_bytes() == m2l
    a.cache_mode_free()
    others_unchanged()
    # new coefficients drop the blocks; fresh ones serve the new medium
    a.cache_mode_near(1)
    assert a.cache_mode_near_bytes() == one
    a.setCoeff(*_coeffs(a.getNodes(), "other"))
    assert a.cache_mode_near_bytes() == 0
    a.cache_block()
    assert a.cache_mode_near_bytes() == 0
    o = _oracle_mode(shape, 1, "other")
    want = np.stack([o.mapping(c, 1) for c in cols])
    a.cache_mode_near(1)
    assert a.cache_mode_near_bytes() == one
    got = _apply(torch, a, cols, 1)
    assert a.mode_apply_calls().tolist() == [8, 4] and _near(a) == ([8, 4], [1, 0])
    worst = max(_rel(got[j], want[j]) for j in range(11))
    print(f"{_ID(shape)} new medium, fresh near blocks vs oracle: {worst:.3e}")
    assert worst <= TOL, worst
    a.cache_mode_near_free()
    assert a.cache_mode_near_bytes() == 0 and a.cache_bytes() == before
