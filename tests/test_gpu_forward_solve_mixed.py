"""The reduced-precision route of a high-order handle on the GPU: the f32
operator entries mapping_multi_f32_dev / forward_multi_f32_dev against the fp64 entries of the
same handle, the float mirrors they read, and forward_solve_multi_mixed(_dev) against the CPU
oracle's gmres_main and the fp64 forward_solve_multi_dev, at the shapes, columns and bounds of
test_gpu_forward_solve_multi.py (S1: np 6, N 1024; S2: np 8, N 1089, W and X lists).

The f32 operator's distance from the fp64 one, relative 2-norm per column, is held between
1e-10 (the fp32 route really ran) and OP_BOUND = 10x the largest value of the first green
run, itself below the cap of 1e-4 that refinement needs to gain four digits per outer step.
First green run, largest per shape over modes 0, 1, 2ks - 2 and nrhs 1, 3, 5, 8, 11:
S1 2.347e-07, S2 3.449e-07; OP_BOUND = 3.5e-6.

Observed refinements (outer) at restart 80, tol 1e-12, inner_tol 1e-4: 3 for every column of S1 (43 .. 56
inner steps; the fp64 solve takes 23 .. 36) and of S2 (21 inner steps; 17), 4 from a random
guess on S2 (27 inner steps); 1 at inner_tol 0.5, max_outer 1 (1 .. 3 inner steps, relres
0.28 .. 0.49)."""
import functools

import numpy as np
import pytest

import test_gpu_forward_solve_multi as fs
from test_gpu_forward_solve_multi import S1, S2, TOL, XTOL

pytestmark = pytest.mark.gpu

OP_FLOOR = 1e-10
OP_CAP = 1e-4
OP_BOUND = 3.5e-6  # 10x the first green run's largest (docstring), never above OP_CAP
assert OP_BOUND <= OP_CAP
NRHS = (1, 3, 5, 8, 11)
SHAPES = pytest.mark.parametrize("shape", [S1, S2], ids=["S1", "S2"])


def _modes(shape):
    return (0, 1, 2 * shape[3] - 2)


def _fresh(shape):
    """A handle of its own (the mirrors' life is what the test is about)."""
    import aniso_amd

    np_, sz, d, ks, ns, ml, coeffs = shape
    a = aniso_amd.Aniso(sz, d, ks, fs.G, ns, np_, ml)
    a.setCoeff(*fs._coeffs(a.getNodes(), coeffs))
    a.cache_block()
    return a


def _rels(got, ref):
    return [fs._rel(got[c], ref[c]) for c in range(ref.shape[0])]


@functools.lru_cache(maxsize=None)
def _fp64_solve(shape, kind, n):
    """forward_solve_multi_dev on the first n columns: (X, iters)."""
    torch = fs._torch()
    a = fs._handle(shape)
    Qd = torch.tensor(fs._columns(shape, kind)[:n], device="cuda")
    X = torch.zeros(n, a.N, dtype=torch.float64, device="cuda")
    iters, relres, _ = a.forward_solve_multi_dev(Qd, X, restart=80, tol=TOL, maxit=5)
    torch.cuda.synchronize()
    assert np.all(iters > 0) and np.all(relres <= TOL)
    x = X.cpu().numpy()
    x.setflags(write=False)
    return x, iters


def _residuals(torch, a, Qd, Xd, rhs_is_source=True):
    """|b - A x| / |b| per column through the fp64 entries."""
    n, N = Qd.shape[0], a.N
    B = torch.zeros(n, N, dtype=torch.float64, device="cuda")
    if rhs_is_source:
        a.mapping_multi_dev(Qd, 0, B)
    else:
        B.copy_(Qd[:, :N])
    F = torch.zeros(n, N, dtype=torch.float64, device="cuda")
    a.forward_multi_dev(Xd[:, :N].contiguous(), F)
    torch.cuda.synchronize()
    b, r = B.cpu().numpy(), (B - F).cpu().numpy()
    return np.array([np.linalg.norm(r[c]) / np.linalg.norm(b[c]) for c in range(n)])


# ---- 1. the f32 operator against the fp64 entry

@SHAPES
def test_f32_operator_against_the_fp64_entry(shape):
    """Modes 0, 1, 2ks - 2 and nrhs 1, 3, 5, 8, 11, rows at stride N + 7 with NaN in the gaps
    and two rows behind the columns: every column of mapping_multi_f32_dev between OP_FLOOR
    and OP_BOUND from mapping_multi_dev; forward_multi_f32_dev within OP_BOUND of
    x - mapping_f32(sigma_s x, 0); gaps, the rows behind and the input untouched."""
    torch = fs._torch()
    a = fs._handle(shape)
    N = a.N
    ss, _ = fs._coeffs(fs._oracle(shape).getNodes(), shape[6])
    Q = fs._columns(shape, "random")
    worst = 0.0
    for nrhs in NRHS:
        xwhole, Xd = fs._rows(torch, Q[:nrhs], extra=2)
        xwhole[nrhs:] = 5.0
        for id_ in _modes(shape):
            ref = torch.zeros(nrhs, N, dtype=torch.float64, device="cuda")
            a.mapping_multi_dev(Xd, id_, ref)
            owhole, Od = fs._rows(torch, np.zeros((nrhs, N)), extra=2)
            owhole[nrhs:] = 7.0
            a.mapping_multi_f32_dev(Xd, id_, Od)
            torch.cuda.synchronize()
            got = owhole.cpu().numpy()
            assert np.all(np.isnan(got[:nrhs, N:])) and np.all(got[nrhs:] == 7.0)
            errs = _rels(got[:nrhs, :N], ref.cpu().numpy())
            worst = max(worst, max(errs))
            print(f"np {shape[0]} mode {id_} nrhs {nrhs}: f32 vs fp64 {min(errs):.3e} .. {max(errs):.3e}")
            assert min(errs) >= OP_FLOOR and max(errs) <= OP_BOUND, (id_, nrhs, errs)
            assert list(a.mode_apply_calls()) == ([8] if nrhs > 8 else []) + [{1: 2, 3: 4, 5: 5, 8: 8, 11: 4}[nrhs]]
        # the forward form
        owhole, Od = fs._rows(torch, np.zeros((nrhs, N)), extra=2)
        owhole[nrhs:] = 7.0
        a.forward_multi_f32_dev(Xd, Od)
        sx = torch.tensor(Q[:nrhs] * ss, device="cuda")
        m = torch.zeros(nrhs, N, dtype=torch.float64, device="cuda")
        a.mapping_multi_f32_dev(sx, 0, m)
        torch.cuda.synchronize()
        got = owhole.cpu().numpy()
        assert np.all(np.isnan(got[:nrhs, N:])) and np.all(got[nrhs:] == 7.0)
        errs = _rels(got[:nrhs, :N], Q[:nrhs] - m.cpu().numpy())
        print(f"np {shape[0]} nrhs {nrhs}: forward form vs x - mapping_f32(sigma_s x, 0) {max(errs):.3e}")
        assert max(errs) <= OP_BOUND, (nrhs, errs)
        xgot = xwhole.cpu().numpy()
        assert np.all(np.isnan(xgot[:nrhs, N:])) and np.all(xgot[nrhs:] == 5.0) and np.array_equal(xgot[:nrhs, :N], Q[:nrhs])
    print(f"np {shape[0]}: largest f32 vs fp64 distance {worst:.3e}")


@SHAPES
def test_f32_columns_are_independent_and_calls_repeat_bitwise(shape):
    """A column alone, beside one other in either slot, and first and last of 11: equal bits;
    a repeated call: equal bits."""
    torch = fs._torch()
    a = fs._handle(shape)
    N = a.N
    Q = torch.tensor(fs._columns(shape, "random"), device="cuda")

    def run(rows, id_, forward):
        X = Q[rows].contiguous()
        out = torch.zeros(len(rows), N, dtype=torch.float64, device="cuda")
        if forward:
            a.forward_multi_f32_dev(X, out)
        else:
            a.mapping_multi_f32_dev(X, id_, out)
        return out

    for id_, forward in [(m, False) for m in _modes(shape)] + [(0, True)]:
        alone = run([4], id_, forward)[0]
        assert torch.equal(run([4, 9], id_, forward)[0], alone)
        assert torch.equal(run([9, 4], id_, forward)[1], alone)
        perm = [4] + [j for j in range(11) if j not in (4,)]
        assert torch.equal(run(perm, id_, forward)[0], alone)
        assert torch.equal(run(perm[1:] + [4], id_, forward)[10], alone)
        whole = run(list(range(11)), id_, forward)
        assert torch.equal(run(list(range(11)), id_, forward), whole)
        assert torch.equal(whole[4], alone)


# ---- 2. the mirrors, and everything else left as it was

@SHAPES
def test_the_mirrors_live_and_die_with_the_shared_caches(shape):
    """cache_f32_bytes: 0 before; after the first f32 call (which builds the mirrors) half the
    bytes of the two E arrays, which is cache_bytes()[1] less sigma_t at every point; 0 after
    setCoeff; after cache_block with the new coefficients the next f32 call is within OP_BOUND
    of the new fp64 operator.  block_op(2), forward_multi_dev and cache_bytes are what they
    were before cache_f32 and after an f32 call."""
    torch = fs._torch()
    a = _fresh(shape)
    N, ks = a.N, a.ks
    U = np.random.default_rng(5).uniform(-1.0, 1.0, (ks, N))
    X = torch.tensor(fs._columns(shape, "random")[:3], device="cuda")

    # (each waits for its launches: block_op, setCoeff and cache_block run on the handle's own
    # stream, which does not order against the caller's)
    def fwd64():
        out = torch.zeros(3, N, dtype=torch.float64, device="cuda")
        a.forward_multi_dev(X, out)
        torch.cuda.synchronize()
        return out

    def map32(id_):
        out = torch.zeros(3, N, dtype=torch.float64, device="cuda")
        a.mapping_multi_f32_dev(X, id_, out)
        torch.cuda.synchronize()
        return out

    def map64(id_):
        out = torch.zeros(3, N, dtype=torch.float64, device="cuda")
        a.mapping_multi_dev(X, id_, out)
        torch.cuda.synchronize()
        return out

    block0, fwd0, bytes0 = a.block_op(2, U), fwd64(), a.cache_bytes()
    assert a.cache_f32_bytes() == 0
    expect = (bytes0[1] - 8 * N) // 2
    assert expect > 0 and (bytes0[1] - 8 * N) % 2 == 0
    old = map32(1)  # builds the mirrors
    assert a.cache_f32_bytes() == expect
    a.cache_f32()   # nothing to do
    assert a.cache_f32_bytes() == expect
    assert a.cache_bytes() == bytes0
    assert np.array_equal(a.block_op(2, U), block0) and torch.equal(fwd64(), fwd0)
    ss, st = fs._coeffs(a.getNodes(), shape[6])
    a.setCoeff(0.5 * ss, 0.5 * st + 0.3)
    assert a.cache_f32_bytes() == 0
    a.cache_block()
    assert a.cache_f32_bytes() == 0
    a.cache_f32()
    assert a.cache_f32_bytes() == expect and a.cache_bytes() == bytes0
    new, ref = map32(1), map64(1)
    torch.cuda.synchronize()
    errs = _rels(new.cpu().numpy(), ref.cpu().numpy())
    moved = _rels(new.cpu().numpy(), old.cpu().numpy())
    print(f"np {shape[0]}: after new coefficients f32 vs fp64 {max(errs):.3e}, vs the old f32 result {min(moved):.3e}")
    assert OP_FLOOR <= min(errs) and max(errs) <= OP_BOUND, errs
    assert min(moved) > 1e-3, moved


# ---- 3. the mixed solve

def _check_passes(calls, groups, outer, nonzero_guess):
    """The pass list of a source-form solve: per group one fp64 pass for the right-hand sides,
    one for a nonzero guess, then per refinement f32 passes and ONE fp64 pass over the columns
    still active."""
    calls = [tuple(int(v) for v in c) for c in calls]
    i = 0
    for g0, ng in groups:
        og = outer[g0:g0 + ng]
        assert calls[i] == (64, ng), (i, calls[i])
        i += 1
        if nonzero_guess:
            assert calls[i][0] == 64, (i, calls[i])
            i += 1
        n64 = 1 + (1 if nonzero_guess else 0)
        for o in range(int(og.max())):
            active = int((og > o).sum())
            n32 = 0
            while calls[i][0] == 32:
                assert 1 <= calls[i][1] <= active
                n32 += 1
                i += 1
            assert n32 >= 1 and calls[i] == (64, active), (o, i, calls[i], active)
            i += 1
            n64 += 1
        assert n64 == 1 + (1 if nonzero_guess else 0) + int(og.max())
    assert i == len(calls), (i, len(calls))


@pytest.mark.parametrize("shape,picks", [(S1, [("mixed", j) for j in range(6)] + [("random", j) for j in range(5)]),
                                         (S2, [("random", j) for j in range(5)])], ids=["S1", "S2"])
def test_every_column_matches_the_oracle_and_the_fp64_solve(shape, picks):
    """restart 80, maxit 5, rhs_is_source, rows at stride N + 7 with NaN in the gaps: every
    column <= XTOL from gmres_main(q, 80, 400, TOL) and from forward_solve_multi_dev, relres <=
    TOL and within 1e-6 (relative) of the residual this test forms through the fp64 entries;
    the pass list has the stated structure; outer >= 1."""
    torch = fs._torch()
    a = fs._handle(shape)
    N = a.N
    Q = np.array([fs._columns(shape, kind)[j] for kind, j in picks])
    n = len(picks)
    qwhole, Qd = fs._rows(torch, Q, extra=2)
    qwhole[n:] = 5.0
    xwhole, Xd = fs._rows(torch, np.zeros((n, N)), extra=2)
    xwhole[n:] = 7.0
    iters, outer, relres = a.forward_solve_multi_mixed_dev(Qd, Xd, restart=80, tol=TOL, maxit=5)
    calls = a.forward_solve_mixed_calls()
    torch.cuda.synchronize()
    got = xwhole.cpu().numpy()
    assert np.all(np.isnan(got[:n, N:])) and np.all(got[n:] == 7.0)
    qgot = qwhole.cpu().numpy()
    assert np.all(np.isnan(qgot[:n, N:])) and np.all(qgot[n:] == 5.0) and np.array_equal(qgot[:n, :N], Q)
    own = _residuals(torch, a, Qd, Xd)
    x64 = {kind: _fp64_solve(shape, kind, 6 if kind == "mixed" else 5)[0] for kind in {k for k, _ in picks}}
    n32, n64 = sum(1 for c in calls if c[0] == 32), sum(1 for c in calls if c[0] == 64)
    print(f"np {shape[0]}: outer {outer.tolist()}, inner steps {iters.tolist()}, passes f32 {n32} fp64 {n64}")
    for c, (kind, j) in enumerate(picks):
        xo = fs._oracle_solve(shape, kind, j, 80)[1]
        eo, e64 = fs._rel(got[c, :N], xo), fs._rel(got[c, :N], x64[kind][j])
        print(f"np {shape[0]} {kind} {j}: {iters[c]} inner steps, outer {outer[c]}, relres {relres[c]:.3e} (own {own[c]:.3e}), "
              f"x vs oracle {eo:.3e}, vs the fp64 solve {e64:.3e}")
        assert iters[c] > 0 and outer[c] >= 1 and relres[c] <= TOL, (c, iters[c], outer[c], relres[c])
        assert abs(own[c] - relres[c]) <= 1e-6 * relres[c], (c, own[c], relres[c])
        assert eo <= XTOL and e64 <= XTOL, (c, eo, e64)
    _check_passes(calls, [(g0, min(8, n - g0)) for g0 in range(0, n, 8)], outer, False)


def test_scaled_sources_give_scaled_solutions():
    torch = fs._torch()
    a = fs._handle(S1)
    N = a.N
    Q = fs._columns(S1, "mixed")[:3]
    x64 = _fp64_solve(S1, "mixed", 6)[0]
    for scale in (1e60, 1e-60):
        X = torch.zeros(3, N, dtype=torch.float64, device="cuda")
        iters, outer, relres = a.forward_solve_multi_mixed_dev(torch.tensor(Q * scale, device="cuda"), X, restart=80,
                                                               tol=TOL, maxit=5)
        torch.cuda.synchronize()
        got = X.cpu().numpy() / scale
        for c in range(3):
            err = fs._rel(got[c], x64[c])
            print(f"scale {scale:g} column {c}: outer {outer[c]}, relres {relres[c]:.3e}, x / scale vs the fp64 solve {err:.3e}")
            assert iters[c] > 0 and relres[c] <= TOL and err <= XTOL, (scale, c, iters[c], relres[c], err)


def test_a_zero_column_in_the_middle_of_five():
    torch = fs._torch()
    a = fs._handle(S2)
    N = a.N
    Q = np.zeros((5, N))
    Q[[0, 1, 3, 4]] = fs._columns(S2, "random")[:4]
    X = torch.zeros(5, N, dtype=torch.float64, device="cuda")
    X[2] = 3.0  # a guess the zero column must overwrite
    iters, outer, relres = a.forward_solve_multi_mixed_dev(torch.tensor(Q, device="cuda"), X, restart=80, tol=TOL, maxit=5)
    torch.cuda.synchronize()
    got = X.cpu().numpy()
    assert iters[2] == 0 and outer[2] == 0 and relres[2] == 0.0 and np.all(got[2] == 0.0)
    x64 = _fp64_solve(S2, "random", 5)[0]
    for c, j in ((0, 0), (1, 1), (3, 2), (4, 3)):
        assert iters[c] > 0 and outer[c] >= 1 and relres[c] <= TOL and fs._rel(got[c], x64[j]) <= XTOL, c
    # only the zero column had a guess, and it needs no pass: the source form's pass structure
    _check_passes(a.forward_solve_mixed_calls(), [(0, 5)], outer, False)


def test_not_converged_keeps_its_refinement_and_reports_its_residual():
    """S1, inner_tol 0.5, max_outer 1: one loose refinement.  iters < 0, tol < relres < 1,
    relres is the fp64 residual of the returned x (1e-6 relative), and x is not the guess."""
    torch = fs._torch()
    a = fs._handle(S1)
    N = a.N
    Qd = torch.tensor(fs._columns(S1, "mixed"), device="cuda")
    X = torch.zeros(6, N, dtype=torch.float64, device="cuda")
    iters, outer, relres = a.forward_solve_multi_mixed_dev(Qd, X, restart=80, tol=TOL, inner_tol=0.5, maxit=5, max_outer=1)
    torch.cuda.synchronize()
    own = _residuals(torch, a, Qd, X)
    for c in range(6):
        print(f"loose column {c}: iters {iters[c]}, outer {outer[c]}, relres {relres[c]:.6e}, own residual {own[c]:.6e}")
        assert iters[c] < 0 and outer[c] == 1, (c, iters[c], outer[c])
        assert TOL < relres[c] < 1.0, (c, relres[c])
        assert abs(own[c] - relres[c]) <= 1e-6 * relres[c], (c, own[c], relres[c])
        assert float(X[c].abs().max()) > 0.0
    _check_passes(a.forward_solve_mixed_calls(), [(0, 6)], outer, False)


def test_initial_guess_and_a_given_right_hand_side():
    torch = fs._torch()
    a = fs._handle(S2)
    N = a.N
    Q = fs._columns(S2, "random")[:3]
    Qd = torch.tensor(Q, device="cuda")
    x64 = _fp64_solve(S2, "random", 5)[0]
    Xg = torch.tensor(np.random.default_rng(3).uniform(-1.0, 1.0, (3, N)), device="cuda")
    iters, outer, relres = a.forward_solve_multi_mixed_dev(Qd, Xg, restart=80, tol=TOL, maxit=5)
    _check_passes(a.forward_solve_mixed_calls(), [(0, 3)], outer, True)
    torch.cuda.synchronize()
    for c in range(3):
        err = fs._rel(Xg[c].cpu().numpy(), x64[c])
        print(f"from a random guess, column {c}: {iters[c]} inner steps, outer {outer[c]}, relres {relres[c]:.3e}, x {err:.3e}")
        assert iters[c] > 0 and relres[c] <= TOL and err <= XTOL, (c, iters[c], relres[c], err)
    X1 = torch.zeros(3, N, dtype=torch.float64, device="cuda")
    it1, ou1, rr1 = a.forward_solve_multi_mixed_dev(Qd, X1, restart=80, tol=TOL, maxit=5, rhs_is_source=True)
    Bd = torch.zeros(3, N, dtype=torch.float64, device="cuda")
    a.mapping_multi_dev(Qd, 0, Bd)
    X0 = torch.zeros(3, N, dtype=torch.float64, device="cuda")
    it0, ou0, rr0 = a.forward_solve_multi_mixed_dev(Bd, X0, restart=80, tol=TOL, maxit=5, rhs_is_source=False)
    torch.cuda.synchronize()
    assert np.array_equal(it0, it1) and np.array_equal(ou0, ou1)
    for c in range(3):
        assert fs._rel(X0[c].cpu().numpy(), X1[c].cpu().numpy()) <= 1e-12, c
    assert int(a.forward_solve_mixed_calls()[0][0]) == 32  # a given b and a zero guess: no fp64 pass before the first solve


def test_host_entry_repeats_and_what_is_left_behind():
    torch = fs._torch()
    a = fs._handle(S2)
    N, ks = a.N, a.ks
    U = np.random.default_rng(5).uniform(-1.0, 1.0, (ks, N))
    first = a.block_op(2, U)
    Q = fs._columns(S2, "random")[:3]
    Xh, ith, ouh, rrh = a.forward_solve_multi_mixed(Q.T, restart=80, tol=TOL, maxit=5)
    assert Xh.shape == (N, 3)
    Qd = torch.tensor(Q, device="cuda")
    X = torch.zeros(3, N, dtype=torch.float64, device="cuda")
    iters, outer, relres = a.forward_solve_multi_mixed_dev(Qd, X, restart=80, tol=TOL, maxit=5)
    again = torch.zeros(3, N, dtype=torch.float64, device="cuda")
    it2, ou2, rr2 = a.forward_solve_multi_mixed_dev(Qd, again, restart=80, tol=TOL, maxit=5)
    torch.cuda.synchronize()
    assert torch.equal(X, again)
    assert np.array_equal(iters, it2) and np.array_equal(outer, ou2) and np.array_equal(relres, rr2)
    assert np.array_equal(ith, iters) and np.array_equal(ouh, outer) and np.array_equal(rrh, relres)
    assert np.array_equal(Xh.T, X.cpu().numpy())
    assert np.array_equal(a.block_op(2, U), first)
