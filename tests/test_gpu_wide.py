"""The wide setting of a high-order handle on the GPU: after set_wide() the
fp64 mode applies form chunks of up to 16 columns on every mode -- k_ho_m2l_mode_wide where the
mode has no stored M2L blocks -- and forward_solve_multi_dev runs lockstep groups of 16.

The anchor: the wide mode M2L keeps k_ho_m2l_mode's thread shape and summation order, and every
launch around it runs at its compiled count as before, so with nothing resident a column's bits
with the setting on are its bits with the setting off -- applies and whole solves.  Against the
CPU oracle at the same order too, column by column; the chunks and near launches of the four
residency states; bits; the solve's operator calls; and the setting's life.

The handles here are this file's own (other files cache handles per shape and expect the
default); the oracle's answers for the first 19 columns are test_gpu_mode_resident.py's."""
import functools

import numpy as np
import pytest

import test_gpu_mode_resident as base
from conftest import gaussian_charge, main_coeffs
from test_gpu_mode_resident import _coeffs, _new_handle, _oracle, _oracle_mode, _rel, _rows, _torch

pytestmark = pytest.mark.gpu

# The route shipped (the routing rule): the orders at which a mode without
# stored M2L blocks forms 16-column chunks with the setting on, i.e. at which the wide mode
# M2L measured shorter than two narrow launches.  At another order such a mode keeps narrow
# chunks; the solve's groups of 16 and a resident mode's chunks do not depend on it.
WIDE_M2L = {6: True, 8: True}

TOL = 1e-10     # the suite's oracle-parity bound
ROUTE = 1e-12   # routes that differ by summation order only
STOL = 1e-12    # the solves' tolerance (main.cpp:141)
NCOL = 25       # 16 + 9: two wide chunks, the second with a padded half

# np, sz, d, ks, ns, maxLevel, coefficients
SHAPES = [
    (6, 32, 1, 3, 10, 20, "demo"),   # N 1024, uniform tree
    (6, 19, 3, 2, 8, 20, "rough"),   # W and X lists, leaves of 9..36 points
    (8, 11, 3, 2, 8, 20, "rough"),   # N 1089, W and X lists
    (8, 32, 1, 3, 10, 20, "demo"),   # uniform tree
    (6, 12, 2, 3, 6, 1, "rough"),    # the root's children are leaves: no V pair, an empty M2L list
]
ROUGH = [SHAPES[1], SHAPES[2]]
# test_gpu_forward_solve_multi.py's S1, the medium of its recipes: there the sources take 23 .. 36
# steps at restart 80 and 66 .. 102 at restart 8 (on the rough shapes every source takes 15 ..
# 19 and all finish in one cycle; on the demo medium GMRES(8) stagnates)
S_MAIN = (6, 32, 1, 3, 10, 20, "main")
_ID = lambda s: f"np{s[0]}sz{s[1]}d{s[2]}ks{s[3]}ml{s[5]}" if isinstance(s, tuple) else str(s)  # noqa: E731


@functools.lru_cache(maxsize=None)
def _handle(shape):
    """This file's handle of the shape: every mode ready, nothing resident, the setting off --
    every test leaves it so."""
    if shape[6] != "main":
        return _new_handle(shape)
    import aniso_amd

    np_, sz, d, ks, ns, ml, _ = shape
    a = aniso_amd.Aniso(sz, d, ks, base.G, ns, np_, ml)
    a.setCoeff(*main_coeffs(a.getNodes()))
    a.cache_block()
    return a


def _reset(a):
    a.set_wide(False)
    a.cache_mode_near_free()
    a.cache_mode_free()


@functools.lru_cache(maxsize=None)
def _columns(N):
    """25 columns: the 19 of test_gpu_mode_resident.py and 6 more."""
    X = np.concatenate([base._columns(N), np.random.default_rng(41 + N).uniform(-1.0, 1.0, (NCOL - base.NCOL, N))])
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def _oracle_columns(shape, m):
    o = _oracle_mode(shape, m)
    N = o.getNodes().shape[0]
    out = np.concatenate([base._oracle_columns(shape, m), np.stack([o.mapping(c, m) for c in _columns(N)[base.NCOL:]])])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _oracle_forward(shape):
    """x - K_0(sigma_s x) of the 25 columns."""
    o = _oracle_mode(shape, 0)
    xy = o.getNodes()
    ss, _ = _coeffs(xy, shape[6])
    out = np.stack([c - o.mapping(ss * c, 0) for c in _columns(xy.shape[0])])
    out.setflags(write=False)
    return out


def _pad(n):
    return {1: 2, 2: 2, 3: 4, 4: 4, 5: 5, 6: 8, 7: 8, 8: 8}[n]


def _chunks(n, wide):
    """mode_apply_calls of n columns: one chunk of 16 whenever more than 8 remain (wide), else
    chunks of 8 with the remainder padded to 2, 4, 5 or 8."""
    out = []
    while n > 0:
        if wide and n > 8:
            out.append(16)
            n -= min(16, n)
        else:
            out.append(_pad(min(8, n)))
            n -= min(8, n)
    return out


def _near_launches(n, wide, near_resident):
    """mode_near_calls of n columns as (columns, flags): a wide chunk is one 16-column launch on
    resident near blocks and otherwise two halves; a narrow launch runs on the stored blocks
    iff they exist and it is a full 8 columns."""
    cols = []
    while n > 0:
        if wide and n > 8:
            cols += [16] if near_resident else [8, _pad(min(8, n - 8))]
            n -= min(16, n)
        else:
            cols.append(_pad(min(8, n)))
            n -= min(8, n)
    return cols, [1 if near_resident and c in (8, 16) else 0 for c in cols]


def _near(a):
    c = a.mode_near_calls()
    return c[:, 0].tolist(), c[:, 1].tolist()


def _apply(torch, a, cols, m):
    out = torch.zeros(cols.shape[0], a.N, dtype=torch.float64, device="cuda")
    a.mapping_multi_dev(torch.tensor(cols, device="cuda"), m, out)
    torch.cuda.synchronize()
    return out.cpu().numpy()


# ---- 1. applies, nothing resident

@pytest.mark.parametrize("nrhs", [9, 11, 13, 14, 16, 19, 25])
@pytest.mark.parametrize("shape", SHAPES, ids=_ID)
def test_wide_applies_match_the_oracle_and_the_narrow_chunks_bit_for_bit(shape, nrhs):
    """Modes 0, 1 (odd: the sign of a transposed block) and 2; second halves of 1 -> 2, 3 -> 4, 5,
    6 -> 8 (zero-padded to the full half) and 8 columns, then [16, 4] and [16, 16] with a padded half.  Rows of stride N + 7 in and
    N + 3 out with NaN in the gaps.  Every column <= 1e-10 from the oracle at the same order
    and bitwise what the same call gives with the setting off; the chunks are those of the
    route; the gaps and x are left alone.  forward_multi_dev likewise."""
    torch = _torch()
    a = _handle(shape)
    _reset(a)
    N = a.N
    cols = _columns(N)[:nrhs]
    wide = WIDE_M2L[shape[0]]

    def call(m):
        X = _rows(torch, cols, 7)
        Out = _rows(torch, np.zeros((nrhs, N)), 3)
        if m is None:
            a.forward_multi_dev(X, Out)
        else:
            a.mapping_multi_dev(X, m, Out)
        torch.cuda.synchronize()
        got, x = Out.cpu().numpy(), X.cpu().numpy()
        assert np.all(np.isnan(got[:, N:])), m
        assert np.all(np.isnan(x[:, N:])) and np.array_equal(x[:, :N], cols), m
        return got[:, :N], a.mode_apply_calls().tolist()

    try:
        for m in (0, 1, 2, None):
            a.set_wide(False)
            off, calls_off = call(m)
            assert calls_off == _chunks(nrhs, False), (m, calls_off)
            a.set_wide(True)
            on, calls_on = call(m)
            assert calls_on == _chunks(nrhs, wide), (m, calls_on)
            want = _oracle_forward(shape) if m is None else _oracle_columns(shape, m)
            worst = max(_rel(on[j], want[j]) for j in range(nrhs))
            print(f"{_ID(shape)} mode {m} nrhs {nrhs}: chunks {calls_on}, worst column vs oracle {worst:.3e}")
            assert not np.any(np.isnan(on)), m
            assert worst <= TOL, (m, worst)
            for j in range(nrhs):
                assert np.array_equal(on[j], off[j]), (m, j, _rel(on[j], off[j]))
    finally:
        _reset(a)


# ---- 2. the four residency states

@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[3]], ids=_ID)
def test_the_chunks_and_near_launches_of_the_four_residency_states(shape):
    """19 columns on mode 1 with the setting on: nothing resident, M2L blocks, near blocks, both.
    With M2L blocks resident the chunks are [16, 4] and the output is bitwise the setting-off
    one (that route is unchanged); without them the chunks are the shipped route's, bitwise the
    setting-off output with nothing resident, and within 1e-12 of it with the near blocks (the
    second half's near field changes route: one 16-column launch on the stored blocks)."""
    torch = _torch()
    a = _handle(shape)
    _reset(a)
    cols = _columns(a.N)[:19]
    m = 1
    routed = WIDE_M2L[shape[0]]
    try:
        for m2l, near in ((False, False), (True, False), (False, True), (True, True)):
            _reset(a)
            if m2l:
                a.cache_mode(m)
            if near:
                a.cache_mode_near(m)
            off = _apply(torch, a, cols, m)
            assert a.mode_apply_calls().tolist() == _chunks(19, m2l)
            a.set_wide(True)
            on = _apply(torch, a, cols, m)
            wide = m2l or routed
            assert a.mode_apply_calls().tolist() == _chunks(19, wide), (m2l, near, a.mode_apply_calls())
            assert _near(a) == _near_launches(19, wide, near), (m2l, near, _near(a))
            worst = max(_rel(on[j], off[j]) for j in range(19))
            print(f"{_ID(shape)} M2L blocks {m2l}, near blocks {near}: worst column on vs off {worst:.3e}")
            if m2l or not near:
                assert np.array_equal(on, off), (m2l, near, worst)
            else:
                assert worst <= ROUTE, worst
            _apply(torch, a, cols[:11], 0)   # another mode: the setting does not depend on the mode
            assert a.mode_apply_calls().tolist() == _chunks(11, routed)
        if routed:
            _reset(a)
            a.set_wide(True)
            _apply(torch, a, cols, m)
            assert a.mode_apply_calls().tolist() == [16, 4] and _near(a) == ([8, 8, 4], [0, 0, 0])
            a.cache_mode_near(m)
            _apply(torch, a, cols, m)
            assert a.mode_apply_calls().tolist() == [16, 4] and _near(a) == ([16, 4], [1, 0])
        # the f32 entry keeps chunks of 8
        Out = torch.zeros(11, a.N, dtype=torch.float64, device="cuda")
        a.mapping_multi_f32_dev(torch.tensor(cols[:11], device="cuda"), m, Out)
        torch.cuda.synchronize()
        assert a.mode_apply_calls().tolist() == [8, 4]
    finally:
        _reset(a)


# ---- 3. bits

@pytest.mark.parametrize("shape", ROUGH, ids=_ID)
def test_repeats_are_bitwise_equal_and_columns_do_not_meet(shape):
    """Nothing resident, the setting on, 16 columns: two identical calls give equal bits, and a
    column's bits do not change when the other 15 are replaced (one column of each half)."""
    torch = _torch()
    a = _handle(shape)
    _reset(a)
    cols = _columns(a.N)[:16]
    other = np.random.default_rng(99).uniform(-3.0, 3.0, cols.shape)
    try:
        a.set_wide(True)
        for m in (1, 2):
            first = _apply(torch, a, cols, m)
            assert a.mode_apply_calls().tolist() == _chunks(16, WIDE_M2L[shape[0]])
            assert np.array_equal(first, _apply(torch, a, cols, m)), m
            for keep in (3, 12):
                mixed = other.copy()
                mixed[keep] = cols[keep]
                assert np.array_equal(_apply(torch, a, mixed, m)[keep], first[keep]), (m, keep)
    finally:
        _reset(a)


# ---- 4. the solve, nothing resident

@functools.lru_cache(maxsize=None)
def _sources(shape, n=19):
    """The "mixed" and "random" recipes of test_gpu_forward_solve_multi.py: six sources of
    different kinds (different step counts) and n - 6 of white noise."""
    xy = _oracle(shape).getNodes()
    N = xy.shape[0]
    rng = np.random.default_rng(11 + N)
    x, y = xy[:, 0], xy[:, 1]
    mixed = np.array([gaussian_charge(xy), rng.uniform(-1.0, 1.0, N),
                      np.exp(-200.0 * ((x - 0.2) ** 2 + (y - 0.7) ** 2)), np.ones(N),
                      1e-3 * rng.uniform(-1.0, 1.0, N), (x > 0.5).astype(np.float64)])
    Q = np.concatenate([mixed, rng.uniform(-1.0, 1.0, (n - 6, N))])
    Q.setflags(write=False)
    return Q


@functools.lru_cache(maxsize=None)
def _sources_16(shape):
    """16 sources of which at least half stop early: the six "mixed" ones, five Gaussians of other
    widths and centres (smooth sources take fewer steps than white noise), five of white noise."""
    xy = _oracle(shape).getNodes()
    x, y = xy[:, 0], xy[:, 1]
    smooth = np.array([np.exp(-w * ((x - cx) ** 2 + (y - cy) ** 2)) for w, cx, cy in
                       ((10.0, 0.5, 0.5), (20.0, 0.3, 0.4), (40.0, 0.6, 0.6), (60.0, 0.7, 0.3), (100.0, 0.4, 0.8))])
    Q = np.concatenate([_sources(shape)[:6], smooth, _sources(shape)[6:11]])
    Q.setflags(write=False)
    return Q


def _solve(torch, a, Q, restart, maxit, guess=None, **kw):
    X = torch.zeros(Q.shape[0], a.N, dtype=torch.float64, device="cuda") if guess is None else torch.tensor(guess, device="cuda")
    iters, relres, hist = a.forward_solve_multi_dev(torch.tensor(Q, device="cuda"), X, restart=restart, tol=STOL,
                                                    maxit=maxit, **kw)
    torch.cuda.synchronize()
    return X.cpu().numpy(), iters, relres, hist, list(a.forward_solve_calls())


def _same_solve(on, off):
    return all(np.array_equal(p, q) for p, q in zip(on[:4], off[:4]))


@pytest.mark.parametrize("restart,maxit", [(80, 5), (8, 60)], ids=["restart80", "restart8"])
@pytest.mark.parametrize("shape", [S_MAIN, SHAPES[2]], ids=_ID)
def test_a_16_source_solve_is_the_narrow_solve_bit_for_bit(shape, restart, maxit):
    """16 sources whose step counts differ, so the live set passes through 16 -> <= 8 inside a
    cycle; restart 80 (one cycle) and restart 8 (columns finish in different cycles, the
    residual call runs on 16 rows).  x, iters, relres and hist are bitwise the setting-off
    solve's.  The operator calls: the first on 16 rows; at restart 80 step j on exactly the
    columns with more than j steps and the explicit residuals on all 16; at restart 8 the
    first cycle is eight 16-row steps and a 16-row residual call; in total the rows of the
    setting-off solve's calls."""
    torch = _torch()
    a = _handle(shape)
    _reset(a)
    Q = _sources_16(shape)
    try:
        off = _solve(torch, a, Q, restart, maxit)
        assert max(off[4]) <= 8, off[4]
        a.set_wide(True)
        on = _solve(torch, a, Q, restart, maxit)
    finally:
        _reset(a)
    iters, calls = on[1], on[4]
    print(f"{_ID(shape)} restart {restart}: steps {iters.tolist()}, {len(calls)} calls on {sum(calls)} rows "
          f"({len(off[4])} calls with the setting off)")
    assert np.all(iters > 0) and np.all(on[2] <= STOL), (iters, on[2])
    assert len(set(iters.tolist())) > 1, iters
    assert _same_solve(on, off), [_rel(on[0][c], off[0][c]) for c in range(16)]
    assert calls[0] == 16 and max(calls) == 16 and sum(calls) == sum(off[4]), (calls, off[4])
    if restart == 80:
        assert np.all(iters <= 80)
        assert calls == [int((iters > j).sum()) for j in range(int(iters.max()))] + [16], (calls, iters)
    else:
        assert np.all(iters > 8) and calls[:9] == [16] * 9, (iters, calls[:9])
    if shape == S_MAIN:
        # the live set did pass through 16 -> <= 8 inside a cycle: narrow chunks inside the group of 16
        assert 0 < min(calls) <= 8, calls
        if restart == 8:
            assert len({(int(i) - 1) // 8 for i in iters}) > 1, iters  # they did finish in different cycles


def test_19_sources_are_groups_of_16_and_3():
    torch = _torch()
    shape = SHAPES[2]
    a = _handle(shape)
    _reset(a)
    Q = _sources(shape)
    try:
        off = _solve(torch, a, Q, 80, 5)
        a.set_wide(True)
        on = _solve(torch, a, Q, 80, 5)
    finally:
        _reset(a)
    assert _same_solve(on, off)
    iters, calls = on[1], on[4]
    first = [int((iters[:16] > j).sum()) for j in range(int(iters[:16].max()))] + [16]
    second = [int((iters[16:] > j).sum()) for j in range(int(iters[16:].max()))] + [3]
    assert calls == first + second, (calls, iters)


def test_a_zero_column_a_given_guess_and_a_solve_that_stops_short():
    """As test_gpu_forward_solve_multi.py pins them, in a group of 16: an all-zero column (with a
    guess it must overwrite) gives x = 0, iters = 0, relres = 0 and an empty history; a column
    with a random guess converges to the zero-guess solution (<= 1e-10); at restart 8, maxit 2
    every white-noise column stops at iters = -16 with relres < 1 (full GMRES needs 17 steps
    there).  All bitwise the setting-off solve's."""
    torch = _torch()
    shape = SHAPES[2]
    a = _handle(shape)
    _reset(a)
    N = a.N
    Q = np.array(_sources(shape)[:16])
    Q[5] = 0.0
    guess = np.zeros((16, N))
    guess[5] = 3.0
    guess[9] = np.random.default_rng(3).uniform(-1.0, 1.0, N)
    noise = np.array(_sources(shape)[6:19])
    noise = np.concatenate([noise, noise[:3][::-1] * 0.5])
    noise[7] = 0.0
    try:
        off = _solve(torch, a, Q, 80, 5, guess=guess)
        plain = _solve(torch, a, Q, 80, 5)
        short_off = _solve(torch, a, noise, 8, 2)
        a.set_wide(True)
        on = _solve(torch, a, Q, 80, 5, guess=guess)
        short_on = _solve(torch, a, noise, 8, 2)
    finally:
        _reset(a)
    assert _same_solve(on, off) and _same_solve(short_on, short_off)
    x, iters, relres, hist, calls = on
    assert iters[5] == 0 and relres[5] == 0.0 and np.all(x[5] == 0.0) and np.all(hist[5] == 0.0)
    live = [c for c in range(16) if c != 5]
    assert np.all(iters[live] > 0) and np.all(relres[live] <= STOL), (iters, relres)
    assert _rel(x[9], plain[0][9]) <= TOL
    # the first residual takes an operator row only for the column whose guess is not zero
    assert calls[0] == 1 and calls[1] == 15, calls[:3]
    x, iters, relres, hist, calls = short_on
    assert iters[7] == 0 and relres[7] == 0.0 and np.all(x[7] == 0.0)
    for c in range(16):
        if c != 7:
            assert iters[c] == -16 and 0.0 < relres[c] < 1.0 and np.all(hist[c, :16] > 0.0), (c, iters[c], relres[c])
    assert calls == [15] * 8 + [15] + [15] * 8 + [15], calls


# ---- 5. the solve, both kinds of blocks resident

@pytest.mark.parametrize("shape", ROUGH, ids=_ID)
def test_a_16_source_solve_on_resident_blocks(shape):
    """Mode 0's M2L and near blocks resident, the setting on: every column converges with
    relres <= tol, the solutions are within 1e-10 of the setting-off solve's (the routes differ
    by summation order only), and the residual recomputed with forward_multi_dev is
    <= 1e-10 |b| (test_forward_form_and_solve_on_resident_mode_0's bound)."""
    torch = _torch()
    a = _handle(shape)
    _reset(a)
    N = a.N
    Q = _sources(shape)[:16]
    try:
        a.cache_mode(0)
        a.cache_mode_near(0)
        off = _solve(torch, a, Q, 80, 5)
        a.set_wide(True)
        on = _solve(torch, a, Q, 80, 5)
        assert on[4][0] == 16 and max(off[4]) <= 8
        assert a.mode_apply_calls().tolist() == [16] and _near(a) == ([16], [1])   # (the last call: the residuals)
        Qd = torch.tensor(Q, device="cuda")
        B = torch.zeros(16, N, dtype=torch.float64, device="cuda")
        a.mapping_multi_dev(Qd, 0, B)
        AU = torch.zeros(16, N, dtype=torch.float64, device="cuda")
        a.forward_multi_dev(torch.tensor(on[0], device="cuda"), AU)
        torch.cuda.synchronize()
    finally:
        _reset(a)
    r, b = (AU - B).cpu().numpy(), B.cpu().numpy()
    assert np.all(on[1] > 0) and np.all(on[2] <= STOL), (on[1], on[2])
    for c in range(16):
        e = _rel(on[0][c], off[0][c])
        rr = float(np.linalg.norm(r[c]) / np.linalg.norm(b[c]))
        print(f"{_ID(shape)} source {c}: {on[1][c]} steps ({off[1][c]} off), relres {on[2][c]:.3e}, "
              f"recomputed {rr:.3e}, x on vs off {e:.3e}")
        assert e <= TOL, (c, e)
        assert rr <= 1e-10, (c, rr)


# ---- 6. life

@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[2]], ids=_ID)
def test_the_life_of_the_setting(shape):
    """On a handle of its own: the setting survives setCoeff, a cache rebuild and the free calls;
    cache_bytes and block_op(2) are unchanged by a wide solve; the host entries equal the device
    entries bit for bit; after set_wide(False) outputs and call lists are what they were before."""
    torch = _torch()
    np_, ks = shape[0], shape[3]
    a = _new_handle(shape, "other")
    N = a.N
    routed = WIDE_M2L[np_]
    cols = _columns(N)[:19]
    Q = _sources(shape)[:11]
    U = np.random.default_rng(5).uniform(-1.0, 1.0, (ks, N))
    assert a.wide is False
    before = _apply(torch, a, cols, 1)
    before_calls = (a.mode_apply_calls().tolist(), _near(a))
    solve_before = _solve(torch, a, Q, 80, 5)
    block, bytes_before = a.block_op(2, U), a.cache_bytes()
    a.set_wide(True)
    a.setCoeff(*_coeffs(a.getNodes(), shape[6]))   # new coefficients drop the caches, not the setting
    assert a.wide is True
    a.cache_block()
    a.cache_mode(0)
    a.cache_mode_near(0)
    a.cache_mode_free()
    a.cache_mode_near_free()
    assert a.wide is True and a.cache_mode_bytes() == 0 and a.cache_mode_near_bytes() == 0
    # the new medium on wide chunks, against the oracle and the host entry
    got = _apply(torch, a, cols, 1)
    assert a.mode_apply_calls().tolist() == _chunks(19, routed)
    assert max(_rel(got[j], _oracle_columns(shape, 1)[j]) for j in range(19)) <= TOL
    host = a.mapping_multi(cols.T, 1)
    assert a.mode_apply_calls().tolist() == _chunks(19, routed)
    assert np.array_equal(host.T, got)
    # back to the first medium: a wide solve leaves the block operator and the caches alone
    a.setCoeff(*_coeffs(a.getNodes(), "other"))
    a.cache_block()
    assert a.wide is True
    wide_solve = _solve(torch, a, Q, 80, 5)
    assert wide_solve[4][0] == 11 and _same_solve(wide_solve, solve_before)
    Xh, ith, rrh = a.forward_solve_multi(Q.T, restart=80, tol=STOL, maxit=5)
    assert np.array_equal(Xh.T, wide_solve[0]) and np.array_equal(ith, wide_solve[1]) and np.array_equal(rrh, wide_solve[2])
    assert a.cache_bytes() == bytes_before and np.array_equal(a.block_op(2, U), block)
    a.set_wide(False)
    assert a.wide is False
    assert np.array_equal(_apply(torch, a, cols, 1), before)
    assert (a.mode_apply_calls().tolist(), _near(a)) == before_calls
    again = _solve(torch, a, Q, 80, 5)
    assert _same_solve(again, solve_before) and again[4] == solve_before[4]
