"""High-order handles (np = 6, 8) on the GPU: single-mode mapping, the
aniso.m block operator, its passes and its solve on the mode-shared caches at Chebyshev
rank 36 / 64, against the CPU oracle at the same order; the accuracy the order buys,
against the oracle's own FMM error; the direct forms across orders; repeatability and
the entry points a high-order handle refuses."""
import functools

import numpy as np
import pytest

from conftest import gaussian_charge, main_coeffs, rough_coeffs

pytestmark = pytest.mark.gpu

TOL = 1e-10  # the suite's oracle-parity bound
G = 0.8


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
def _handle(sz, d, ks, ns, np_, coeffs, how="block", ml=20):
    """A device handle with every mode ready: `how` = "block" (aniso_cache_block) or
    "modes" (aniso_cache(id) per mode).  Built once per shape, left as found."""
    import aniso_amd

    a = aniso_amd.Aniso(sz, d, ks, G, ns, np_, ml)
    a.setCoeff(*_coeffs(a.getNodes(), coeffs))
    if how == "block":
        a.cache_block()
    else:
        for m in range(2 * ks - 1):
            a.cache(m)
    return a


@functools.lru_cache(maxsize=None)
def _oracle(sz, d, ks, ns, np_, coeffs, modes, ml=20):
    from oracle.oracle_py import Oracle

    o = Oracle(sz, d, ks, G, ns, np_, ml)
    o.setCoeff(*_coeffs(o.getNodes(), coeffs))
    for m in modes:
        o.cache(m)
    return o


@functools.lru_cache(maxsize=None)
def _xy(sz, d):
    import aniso_amd

    xy = aniso_amd.Aniso(sz, d, 1, G, 6, 4, 0).getNodes()
    xy.setflags(write=False)
    return xy


@functools.lru_cache(maxsize=None)
def _charge(sz, d, coeffs):
    """sigma_s .* (gaussian + U(-0.1, 0.1))."""
    xy = _xy(sz, d)
    ss, _ = _coeffs(xy, coeffs)
    q = ss * (gaussian_charge(xy) + np.random.default_rng(sz * 10 + d).uniform(-0.1, 0.1, xy.shape[0]))
    q.setflags(write=False)
    return q


@functools.lru_cache(maxsize=None)
def _oracle_mapping(sz, d, ks, ns, np_, coeffs, modes, m, ml=20):
    out = _oracle(sz, d, ks, ns, np_, coeffs, modes, ml).mapping(_charge(sz, d, coeffs), m)
    out.setflags(write=False)
    return out


def _block_input(ks, N, seed=5):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (ks, N))


def _block_ref(o, U, g, ss, which):
    """aniso.m forward / mforward / x - mforward(x) composed from oracle mode applies."""
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


# ---- 1. mapping parity

# sz, d, ks, ns, coefficients, how the modes are made ready
SHAPES = [
    (32, 1, 3, 10, "demo", "block"),
    (48, 1, 2, 10, "main", "modes"),
    (11, 3, 2, 8, "rough", "block"),   # odd sz, a non-uniform tree
    (20, 3, 2, 8, "rough", "modes"),   # np = 6 only
    # np = 6 only: the four shapes above have uniform trees at capacity 36, without W and X
    # lists; the neighbouring (19, 3) has them (20 members each, a tree of depth 4)
    (19, 3, 2, 8, "rough", "block"),
]
CASES = [(6, s) for s in SHAPES] + [(8, s) for s in SHAPES[:3]]


@pytest.mark.parametrize("np_,shape", CASES, ids=lambda c: str(c) if isinstance(c, int) else f"sz{c[0]}d{c[1]}ks{c[2]}{c[5]}")
def test_mapping_matches_the_oracle_at_the_same_order(np_, shape):
    """mapping of modes 0 and 2ks - 2 against Oracle(..., np, ...), relative l2 <= 1e-10,
    host and device entry; the mode made ready by aniso_cache_block or by aniso_cache(id)."""
    torch = _torch()
    sz, d, ks, ns, coeffs, how = shape
    a = _handle(sz, d, ks, ns, np_, coeffs, how)
    q = _charge(sz, d, coeffs)
    modes = (0, 2 * ks - 2)
    assert a.cache_bytes()[0] == 0 and a.cache_bytes()[1] > 0
    for m in modes:
        ref = _oracle_mapping(sz, d, ks, ns, np_, coeffs, modes, m)
        got = a.mapping(q, m)
        err = _rel(got, ref)
        print(f"np {np_} sz {sz} d {d} mode {m} ({how}): rel err vs oracle {err:.3e}")
        assert err <= TOL, (m, err)
        out = torch.zeros(a.N, dtype=torch.float64, device="cuda")
        a.mapping_dev(torch.tensor(q, device="cuda"), m, out)
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), got), m


@pytest.mark.parametrize("np_", [6, 8])
def test_order_4_is_a_different_operator(np_):
    """The np = 4 oracle differs from the np-order oracle by more than 1e-6 on the same
    input (2e-4 at this shape on the CPU), so a path that silently ran rank 16 cannot pass
    the parity test above."""
    _torch()
    sz, d, ks, ns, coeffs, _ = SHAPES[0]
    modes = (0, 2 * ks - 2)
    hi = _oracle_mapping(sz, d, ks, ns, np_, coeffs, modes, 0)
    lo = _oracle_mapping(sz, d, ks, ns, 4, coeffs, modes, 0)
    diff = _rel(lo, hi)
    print(f"np 4 against np {np_} oracle, mode 0: {diff:.3e}")
    assert diff > 1e-6, diff


@pytest.mark.parametrize("np_", [6, 8])
def test_the_shapes_cover_every_far_field_stage(np_):
    """From tree_nodes / tree_list: the shapes of the parity test, taken together, hold a
    tree at least three levels deep (M2M and L2L run), a leaf of more than 16 points (the
    64-lane near field) and non-empty W and X lists."""
    _torch()
    deep = big = w = x = False
    for np_c, (sz, d, ks, ns, coeffs, how) in CASES:
        if np_c != np_:
            continue
        a = _handle(sz, d, ks, ns, np_, coeffs, how)
        ints, _ = a.tree_nodes()
        leaf = ints[:, 7] == 1
        deep = deep or ints[:, 5].max() >= 3
        big = big or ints[leaf, 9].max() > 16
        wp, _ = a.tree_list(2)
        xp, _ = a.tree_list(3)
        w = w or wp[-1] > 0
        x = x or xp[-1] > 0
    assert deep and big and w and x, (deep, big, w, x)


# ---- 2. block operator

@functools.lru_cache(maxsize=None)
def _block_oracle_ref(ks, np_, which):
    sz, d, ns = 32, 1, 10
    o = _oracle(sz, d, ks, ns, np_, "demo", tuple(range(2 * ks - 1)))
    ss, _ = _coeffs(_xy(sz, d), "demo")
    ref = _block_ref(o, _block_input(ks, sz * sz * d * d), G, ss, which)
    ref.setflags(write=False)
    return ref


@pytest.mark.parametrize("which", [0, 1, 2])
@pytest.mark.parametrize("ks", [5, 9])
def test_block_operator_matches_the_composed_oracle(ks, which):
    """aniso.m's forward / mforward / x - mforward(x) at np = 6: ks = 5 is one pass, ks = 9
    runs 2 x 2 passes through the window form of the M2L; against aniso.m's composition of
    oracle mode applies, <= 1e-10; host and device entry agree bitwise."""
    torch = _torch()
    sz, d, ns, np_ = 32, 1, 10, 6
    a = _handle(sz, d, ks, ns, np_, "demo")
    U = _block_input(ks, a.N)
    ref = _block_oracle_ref(ks, np_, which)
    got = a.block_op(which, U)
    err = _rel(got, ref)
    print(f"np {np_} ks {ks} which {which}: rel err vs composed oracle {err:.3e}")
    assert err <= TOL, err
    out = torch.zeros(ks, a.N, dtype=torch.float64, device="cuda")
    a.block_op_dev(which, torch.tensor(U, device="cuda"), out)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), got)


def test_block_pass_matches_the_composed_oracle():
    """aniso_block_pass_dev on the np = 6, ks = 9 handle: the four passes of mforward sum
    to the operator (<= 1e-10 against the composed oracle)."""
    torch = _torch()
    import aniso_amd

    sz, d, ns, np_, ks = 32, 1, 10, 6, 9
    a = _handle(sz, d, ks, ns, np_, "demo")
    chunk, P = aniso_amd.block_pass_plan(ks)
    assert (chunk, P) == (8, 2)
    U = torch.tensor(_block_input(ks, a.N), device="cuda")
    acc = np.zeros((P * chunk, a.N))
    for I in range(P):
        for J in range(P):
            out = torch.zeros(chunk, a.N, dtype=torch.float64, device="cuda")
            a.block_pass_dev(1, I, J, U, out)
            torch.cuda.synchronize()
            acc[I * chunk:(I + 1) * chunk] += out.cpu().numpy()
    err = _rel(acc[:ks], _block_oracle_ref(ks, np_, 1))
    print(f"np {np_} ks {ks} passes of mforward: rel err {err:.3e}")
    assert err <= TOL, err
    assert np.all(acc[ks:] == 0.0)


def test_one_block_at_order_8_is_main_cpp_forward_operator():
    """ks = 1, np = 8: which = 2 is main.cpp's u - K_0(sigma_s u) against the oracle."""
    _torch()
    sz, d, ks, ns, np_ = 32, 1, 1, 10, 8
    a = _handle(sz, d, ks, ns, np_, "demo")
    o = _oracle(sz, d, ks, ns, np_, "demo", (0,))
    ss, _ = _coeffs(_xy(sz, d), "demo")
    U = _block_input(1, a.N)
    ref = U[0] - o.mapping(ss * U[0], 0)
    got = a.block_op(2, U)
    err = _rel(got[0], ref)
    print(f"np 8 ks 1 which 2: rel err vs oracle {err:.3e}")
    assert err <= TOL, err
    assert _rel(a.apply_block(U, ss, G)[0], ref) <= TOL


# ---- 3. solve

def test_block_solve_converges_to_the_oracle_operator():
    """block_solve at (32, 1, ks = 3, np = 6), tol 1e-11: it converges, and the residual of
    its solution under the ORACLE-composed operator is <= 1e-9 (the 1e-10 parity bound
    times the iteration's amplification, two digits of room).
    Measured on an MI355X: 55 steps, relres 7.28e-12, oracle-composed residual 7.29e-12."""
    _torch()
    sz, d, ks, ns, np_ = 32, 1, 3, 10, 6
    a = _handle(sz, d, ks, ns, np_, "demo")
    o = _oracle(sz, d, ks, ns, np_, "demo", tuple(range(2 * ks - 1)))
    xy = _xy(sz, d)
    ss, _ = _coeffs(xy, "demo")
    F = np.stack([gaussian_charge(xy) * (0.5 ** b) for b in range(ks)])
    rhs = a.block_op(0, F)
    it, u, hist, relres = a.block_solve(rhs, restart=60, tol=1e-11, maxit=20)
    print(f"block solve: {it} iterations, relres {relres:.3e}")
    assert it > 0 and relres <= 1e-11, (it, relres)
    res = np.linalg.norm(rhs - _block_ref(o, u, G, ss, 2)) / np.linalg.norm(rhs)
    print(f"oracle-composed residual {res:.3e}")
    assert res <= 1e-9, res


# ---- 4. accuracy: the point of the feature

def test_fmm_error_falls_an_order_of_magnitude_per_step():
    """(32, 1, ks = 3, ns = 10), demo.m's coefficients, all N targets: fmm_error(q, 0) on
    np = 4, 6 and 8 handles lies within 2e-10 (absolute: the parity bound on both terms)
    of the FMM oracle's distance from the one-leaf oracle, and falls by more than 10x
    from 4 to 6 and from 6 to 8 (58x and 55x on the CPU)."""
    _torch()
    sz, d, ks, ns, coeffs = 32, 1, 3, 10, "demo"
    q = _charge(sz, d, coeffs)
    modes = (0, 2 * ks - 2)
    leaf = _oracle_mapping(sz, d, ks, ns, 4, coeffs, (0,), 0, 0)  # one leaf: no order enters
    err = {}
    for np_ in (4, 6, 8):
        want = _rel(_oracle_mapping(sz, d, ks, ns, np_, coeffs, modes, 0), leaf)
        a = _handle(sz, d, ks, ns, np_, coeffs)
        l2, mx, t = a.fmm_error(q, 0, ntargets=None)
        print(f"np {np_}: oracle FMM error {want:.6e}, fmm_error {l2:.6e} (max {mx:.3e})")
        assert t.size == a.N
        assert abs(l2 - want) <= 2e-10, (np_, l2, want)
        err[np_] = l2
    assert err[6] < err[4] / 10 and err[8] < err[6] / 10, err
    U = _block_input(ks, sz * sz)
    b6 = _handle(sz, d, ks, ns, 6, coeffs).block_fmm_error(2, U, ntargets=64)[0]
    b4 = _handle(sz, d, ks, ns, 4, coeffs).block_fmm_error(2, U, ntargets=64)[0]
    print(f"block which=2 fmm error: np 4 {b4:.3e}, np 6 {b6:.3e}")
    assert 0 < b6 < b4


# ---- 5. direct forms

def test_direct_forms_do_not_depend_on_the_order():
    """mapping_direct and block_op_direct on an np = 6 handle against an np = 4 handle, same
    geometry and targets, <= 1e-13 (the cross-tree bound: the trees differ, so the
    summation order does and the results are not bitwise equal)."""
    _torch()
    sz, d, ks, ns, coeffs = 11, 3, 2, 8, "rough"
    a6, a4 = _handle(sz, d, ks, ns, 6, coeffs), _handle(sz, d, ks, ns, 4, coeffs)
    q = _charge(sz, d, coeffs)
    t = a6.draw_targets(40, 1)
    for m in (0, 2):
        assert _rel(a6.mapping_direct(q, m, t), a4.mapping_direct(q, m, t)) <= 1e-13, m
    U = _block_input(ks, a6.N)
    for which in (0, 2):
        assert _rel(a6.block_op_direct(which, U, t), a4.block_op_direct(which, U, t)) <= 1e-13, which


# ---- 6. repeatability and refusals

def test_repeatable_and_refusing():
    """Two block_op calls return equal bits; every entry outside a high-order handle's
    scope returns its code with a message, and a following apply still matches."""
    torch = _torch()
    import aniso_amd

    sz, d, ks, ns, np_ = 32, 1, 5, 10, 6
    a = _handle(sz, d, ks, ns, np_, "demo")
    N = a.N
    U = _block_input(ks, N)
    first = a.block_op(2, U)
    assert np.array_equal(a.block_op(2, U), first)
    assert a.cache_bytes()[0] == 0

    def dev(*shape, dtype=torch.float64):
        return torch.zeros(*shape, dtype=dtype, device="cuda")

    q = dev(N)
    refused = [
        ("mapping_batched", lambda: a.mapping_batched(np.ones((N, 2)), 0)),
        ("mapping_tree_dev", lambda: a.mapping_tree_dev(q, 0, dev(N))),
        ("forward_dev", lambda: a.forward_dev(q, dev(N))),
        ("forward_tree_dev", lambda: a.forward_tree_dev(q, dev(N))),
        ("forward_tree_begin_dev", lambda: a.forward_tree_begin_dev(q, dev(N), None)),
        ("forward_tree_end_dev", lambda: a.forward_tree_end_dev(q, dev(N), None, 1)),
        ("gmres", lambda: a.gmres(np.ones(N))),
        ("forward_f32_dev", lambda: a.forward_f32_dev(dev(N, 16, dtype=torch.float32), dev(N, 16, dtype=torch.float32))),
        ("forward16_f64_dev", lambda: a.forward16_f64_dev(dev(N, 16), dev(N, 16))),
        ("mapping16_f64_dev", lambda: a.mapping16_f64_dev(0, dev(N, 16), dev(N, 16))),
        ("solve16_mixed_dev", lambda: a.solve16_mixed_dev(dev(16, N), dev(16, N))),
        ("solve_mixed_dev", lambda: a.solve_mixed_dev(dev(3, N), dev(3, N))),
        ("stage mask", lambda: a.mapping_dev(q, 0, dev(N), mask=aniso_amd.STAGE_ALL & ~2)),
        ("block_op_begin_dev", lambda: a.block_op_begin_dev(2, dev(ks, N), dev(ks, N), None)),
        ("block_op_end_dev", lambda: a.block_op_end_dev(2, dev(ks, N), dev(ks, N), None, 1)),
        ("block_op_sharded_dev", lambda: a.block_op_sharded_dev(2, dev(ks, N), dev(ks, N))),
        ("block_solve_sharded_dev", lambda: a.block_solve_sharded_dev(dev(ks, N), dev(ks, N))),
        ("comm_init_loopback", lambda: a.comm_init_loopback()),
        ("comm_init_rccl", lambda: a.comm_init_rccl(bytes(128))),
    ]
    for name, call in refused:
        with pytest.raises(aniso_amd.AnisoError) as e:
            call()
        assert e.value.code == 3, (name, e.value.code, str(e.value))  # ANISO_ERR_STATE
        assert "high-order" in str(e.value), (name, str(e.value))
    with pytest.raises(aniso_amd.AnisoError) as e:
        a.set_deterministic(True)
    assert e.value.code == 1 and str(e.value)  # ANISO_ERR_INVALID, as for ks > 8
    with pytest.raises(aniso_amd.AnisoError) as e:
        a.set_shard(0, 2)
    assert e.value.code == 1 and str(e.value)
    torch.cuda.synchronize()
    assert np.array_equal(a.block_op(2, U), first)
    assert a.cache_bytes()[0] == 0
