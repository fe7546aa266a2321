"""Lean block handles: aniso_cache_block readies every mode for the
block operator on the mode-shared caches and builds no per-mode operator cache.

Tolerances are the project's own: 1e-10 against the oracle (TOL of
test_gpu_block_passes.py), 1e-13 for the harmonic form against the per-mode stream
(test_one_pass_matches_the_generic_stream), 1e-14 between two default clustered applies
of one operator (test_block_matvec_tree_order_and_shards_compose), and bitwise where
the summation order is fixed (the ks > 8 passes, the deterministic mode)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import gaussian_charge, main_coeffs, rough_coeffs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-10
G = 0.8


def _torch():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def _rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def _block_ref(o, U, g, ss, which):
    """aniso.m forward / mforward / x - mforward(x) composed from oracle mode applies
    (the composition of test_gpu_block_passes.py, restated)."""
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


def _coeffs(xy, coeffs):
    return main_coeffs(xy) if coeffs == "main" else rough_coeffs(xy, 7)


def _handle(sz, d, ks, ns, ml, coeffs, lean):
    """A fresh handle with its coefficients set and every mode made ready: by one
    cache_block() (lean) or by the cache(m) loop."""
    import aniso_amd

    a = aniso_amd.Aniso(sz, d, ks, G, ns, 4, ml)
    a.setCoeff(*_coeffs(a.getNodes(), coeffs))
    if lean:
        a.cache_block()
    else:
        for m in range(2 * ks - 1):
            a.cache(m)
    return a


@functools.lru_cache(maxsize=None)
def _shared(sz, d, ks, ns, ml, coeffs, lean):
    """Handles shared between tests; those tests leave them as they found them."""
    return _handle(sz, d, ks, ns, ml, coeffs, lean)


@functools.lru_cache(maxsize=None)
def _oracle(sz, d, ks, ns, ml, coeffs):
    from oracle.oracle_py import Oracle

    o = Oracle(sz, d, ks, G, ns, 4, ml)
    lean = _shared(sz, d, ks, ns, ml, coeffs, True)
    xy = lean.getNodes()
    ss, st = _coeffs(xy, coeffs)
    o.setCoeff(ss, st)
    for m in range(2 * ks - 1):
        o.cache(m)
    return o, xy, ss


@functools.lru_cache(maxsize=None)
def _input(ks, N, seed):
    U = np.random.default_rng(seed).uniform(-1, 1, (ks, N))
    U.setflags(write=False)
    return U


SHAPES = [
    # sz, d, ks, ns, maxLevel, coeffs
    (16, 1, 5, 8, 20, "main"),
    (12, 2, 3, 8, 20, "rough"),   # padded to 4
    (12, 1, 7, 8, 20, "rough"),   # padded to 8
    (11, 1, 2, 6, 20, "rough"),
    (24, 1, 4, 10, 2, "rough"),   # 64-point leaves
    (16, 1, 9, 8, 20, "main"),
    (10, 2, 16, 8, 20, "rough"),
    (8, 1, 17, 8, 20, "main"),
]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda c: f"sz{c[0]}d{c[1]}ks{c[2]}ns{c[3]}ml{c[4]}{c[5]}")
def test_block_operator_on_a_lean_handle_matches_oracle(shape):
    """setCoeff + cache_block() only: forward, mforward and x - mforward(x) through the
    device and the host entry points against the oracle's composition, <= 1e-10; the
    handle runs the harmonic form and holds no per-mode operator."""
    torch = _torch()
    a = _shared(*shape, True)
    o, xy, ss = _oracle(*shape)
    ks = shape[2]
    U = _input(ks, a.N, shape[0] + ks).copy()
    U[0] += gaussian_charge(xy)
    Ud = torch.tensor(U, device="cuda")
    for which in (0, 1, 2):
        out = torch.zeros_like(Ud)
        a.block_op_dev(which, Ud, out)
        torch.cuda.synchronize()
        ref = _block_ref(o, U, G, ss, which)
        err = _rel(out.cpu().numpy(), ref)
        herr = _rel(a.block_op(which, U.reshape(-1)).reshape(ks, a.N), ref)
        print(f"lean ks={ks} which={which}: device rel err {err:.3e}, host {herr:.3e}")
        assert err <= TOL, (which, err)
        assert herr <= TOL, (which, herr)
    assert a.stats()["harmonic"] == 1
    assert a.cache_bytes()[0] == 0


def _matvec(a, U):
    torch = _torch()
    out = torch.zeros_like(U)
    a.block_op_dev(2, U, out)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("shape", [(12, 1, 12, 8, 20, "rough"), (128, 1, 12, 10, 20, "main")],
                         ids=lambda c: f"sz{c[0]}")
def test_lean_equals_cached_bitwise_beyond_8_blocks(shape):
    """ks = 12: the passes sum in a fixed order and read no per-mode cache, so a lean and
    a fully cached handle give the same bits (the second shape: N = 16,384)."""
    torch = _torch()
    lean, full = _shared(*shape, True), _shared(*shape, False)
    U = torch.tensor(_input(12, lean.N, 5), device="cuda")
    yl, yf = _matvec(lean, U), _matvec(full, U)
    assert torch.isfinite(yl).all() and float(torch.linalg.norm(yl)) > 0
    assert torch.equal(yl, yf), float(torch.linalg.norm(yl - yf) / torch.linalg.norm(yf))


def test_lean_equals_cached_on_the_clustered_launch():
    """ks = 5 at N = 16,384: the clustered, fused launch on a lean handle, <= 1e-14 of
    the cached handle's (two default clustered applies agree to that); bitwise with the
    deterministic sums on both."""
    torch = _torch()
    shape = (128, 1, 5, 10, 20, "main")
    lean, full = _shared(*shape, True), _shared(*shape, False)
    U = torch.tensor(_input(5, lean.N, 6), device="cuda")
    yl, yf = _matvec(lean, U), _matvec(full, U)
    err = float(torch.linalg.norm(yl - yf) / torch.linalg.norm(yf))
    print(f"lean vs cached, clustered ks=5 N={lean.N}: {err:.3e}")
    assert err <= 1e-14, err
    lean.set_deterministic(1)
    full.set_deterministic(1)
    try:
        dl, df = _matvec(lean, U), _matvec(full, U)
    finally:
        lean.set_deterministic(0)
        full.set_deterministic(0)
    assert torch.equal(dl, df)
    assert float(torch.linalg.norm(dl)) > 0
    assert lean.cache_bytes()[0] == 0


def test_lean_mapping_matches_oracle_for_every_mode():
    """mapping(charge, m) on a lean ks = 12 handle, m = 0 .. 22 (three windows of the
    offset form), against the oracle's mapping, <= 1e-10."""
    _torch()
    shape = (12, 1, 12, 8, 20, "rough")
    a = _shared(*shape, True)
    o, xy, _ = _oracle(*shape)
    q = gaussian_charge(xy) + 0.1 * _input(1, a.N, 11)[0]
    for m in range(2 * 12 - 1):
        err = _rel(a.mapping(q, m), o.mapping(q, m))
        print(f"lean mapping mode {m}: rel err vs oracle {err:.3e}")
        assert err <= TOL, (m, err)
    assert a.cache_bytes()[0] == 0


def test_lean_mapping_dev_matches_resident_and_cache_makes_a_mode_resident():
    """ks = 5: mapping_dev on a lean handle against the cached handle's per-mode stream
    for m = 0 .. 8 (m = 8: the second window), <= 1e-13; a stage mask is refused on a
    non-resident mode (code 3); after cache(0) mode 0 takes the resident path, bit for
    bit the cached handle's, and the handle holds exactly one mode's operators."""
    torch = _torch()
    import aniso_amd

    shape = (16, 1, 5, 8, 20, "main")
    lean, full = _handle(*shape, True), _shared(*shape, False)
    q = torch.tensor(gaussian_charge(lean.getNodes()) + 0.1 * _input(1, lean.N, 12)[0], device="cuda")
    for m in range(9):
        got = lean.mapping_dev(q, m, torch.full_like(q, 7.0))
        ref = full.mapping_dev(q, m, torch.zeros_like(q))
        torch.cuda.synchronize()
        err = float(torch.linalg.norm(got - ref) / torch.linalg.norm(ref))
        print(f"lean mapping_dev mode {m}: rel err vs resident {err:.3e}")
        assert err <= 1e-13, (m, err)
    keep = torch.full_like(q, 7.0)
    with pytest.raises(aniso_amd.AnisoError) as e:
        lean.mapping_dev(q, 1, keep, mask=aniso_amd.STAGE_ALL & ~1)
    assert e.value.code == 3 and "aniso_cache(1)" in str(e.value)
    torch.cuda.synchronize()
    assert bool((keep == 7.0).all())
    lean.cache(0)
    got = lean.mapping_dev(q, 0, torch.zeros_like(q))
    ref = full.mapping_dev(q, 0, torch.zeros_like(q))
    torch.cuda.synchronize()
    assert torch.equal(got, ref)
    per_mode, _ = lean.cache_bytes()
    assert per_mode * 9 == full.cache_bytes()[0] and per_mode > 0


def test_block_solve_on_a_lean_handle_is_the_cached_solve():
    """aniso.m:159-173's solve at ks = 10 on a lean handle: the step count and the bits
    of the cached handle's solve (the passes sum in a fixed order)."""
    _torch()
    shape = (11, 1, 10, 6, 20, "rough")
    lean, full = _shared(*shape, True), _shared(*shape, False)
    ks = 10
    charge = np.zeros((ks, lean.N))
    charge[0] = gaussian_charge(lean.getNodes())
    rhs = full.block_op(0, charge.reshape(-1))
    its_f, u_f, _, rr_f = full.block_solve(rhs, 400, 1e-11, 400)
    its_l, u_l, _, rr_l = lean.block_solve(rhs, 400, 1e-11, 400)
    print(f"block solve ks=10: cached {its_f} steps relres {rr_f:.3e}, lean {its_l} steps relres {rr_l:.3e}")
    assert its_f > 0 and rr_f <= 1e-11
    assert its_l == its_f
    assert np.array_equal(u_l, u_f)
    assert lean.cache_bytes()[0] == 0


def test_lean_handle_refuses_what_streams_per_mode_operators():
    """Everything that needs resident operators returns ANISO_ERR_STATE naming
    aniso_cache(id), writes nothing, and leaves the handle usable."""
    torch = _torch()
    import aniso_amd

    shape = (16, 1, 5, 8, 20, "main")
    a = _shared(*shape, True)
    o, xy, ss = _oracle(*shape)
    ks, N = 5, a.N
    v = torch.ones(N, dtype=torch.float64, device="cuda")
    out1 = torch.full((N,), 7.0, dtype=torch.float64, device="cuda")
    X16 = torch.ones(N, 16, dtype=torch.float64, device="cuda")
    Y16 = torch.full((N, 16), 7.0, dtype=torch.float64, device="cuda")
    B16 = torch.ones(16, N, dtype=torch.float64, device="cuda")
    S16 = torch.full((16, N), 7.0, dtype=torch.float64, device="cuda")
    x5 = torch.ones(ks, N, dtype=torch.float64, device="cuda")
    o5 = torch.full((ks, N), 7.0, dtype=torch.float64, device="cuda")
    eye3 = np.stack([np.eye(ks)] * 3)
    calls = {
        "mapping_batched": lambda: a.mapping_batched(np.ones((N, 2)), 0),
        "forward_dev": lambda: a.forward_dev(v, out1),
        "gmres": lambda: a.gmres(np.ones(N)),
        "forward16_f64_dev": lambda: a.forward16_f64_dev(X16, Y16),
        "solve16_mixed_dev": lambda: a.solve16_mixed_dev(B16, S16),
        "apply_block_dev": lambda: a.apply_block_dev(x5, [0, 2, 4], eye3, o5),
    }
    for name, call in calls.items():
        with pytest.raises(aniso_amd.AnisoError) as e:
            call()
        assert e.value.code == 3, (name, str(e.value))
        assert "aniso_cache(" in str(e.value), (name, str(e.value))
    torch.cuda.synchronize()
    for t in (out1, Y16, S16, o5):
        assert bool((t == 7.0).all())
    U = _input(ks, N, 13)
    got = _matvec(a, torch.tensor(U, device="cuda")).cpu().numpy()
    assert _rel(got, _block_ref(o, U, G, ss, 2)) <= TOL
    assert a.cache_bytes()[0] == 0


def test_set_coeff_invalidates_a_lean_handle_until_cache_block():
    """A second setCoeff: the block operator is a state error until cache_block() runs
    again, then it is bit for bit a fresh lean handle's on the new coefficients (ks = 12)."""
    torch = _torch()
    import aniso_amd

    shape = (12, 1, 12, 8, 20, "rough")
    a = _handle(*shape, True)
    xy = a.getNodes()
    U = torch.tensor(_input(12, a.N, 5), device="cuda")
    _matvec(a, U)
    ss2, st2 = rough_coeffs(xy, 21)
    a.setCoeff(ss2, st2)
    keep = torch.full_like(U, 7.0)
    with pytest.raises(aniso_amd.AnisoError) as e:
        a.block_op_dev(2, U, keep)
    assert e.value.code == 3
    with pytest.raises(aniso_amd.AnisoError) as e:
        a.block_solve(np.ones(12 * a.N), 10, 1e-6, 1)
    assert e.value.code == 3
    torch.cuda.synchronize()
    assert bool((keep == 7.0).all())
    a.cache_block()
    fresh = aniso_amd.Aniso(*shape[:3], G, shape[3], 4, shape[4])
    fresh.setCoeff(ss2, st2)
    fresh.cache_block()
    assert torch.equal(_matvec(a, U), _matvec(fresh, U))


def _near_k_total(a):
    """Doubles of one mode's Knear as cache(id) allocates it (Plan::nearKTotal, directed
    storage): per non-empty leaf, its non-empty U and W sources' points times its own
    point count padded to a multiple of 4."""
    ints, _ = a.tree_nodes()
    is_leaf, is_empty, count = ints[:, 7], ints[:, 8], ints[:, 9].astype(np.int64)
    total = 0
    lists = [a.tree_list(0), a.tree_list(2)]
    for i in np.nonzero((is_leaf != 0) & (is_empty == 0))[0]:
        S = 0
        for ptr, idx in lists:
            src = idx[ptr[i]:ptr[i + 1]]
            S += int(count[src[is_empty[src] == 0]].sum())
        total += S * ((int(count[i]) + 3) & ~3)
    return total


@pytest.mark.parametrize("shape", [(12, 1, 5, 8, 20, "rough"), (11, 2, 3, 6, 20, "rough")], ids=lambda c: f"sz{c[0]}d{c[1]}")
def test_cache_bytes_accounts_for_what_each_handle_holds(shape):
    _torch()
    ks = shape[2]
    full, lean = _handle(*shape, False), _shared(*shape, True)
    st = full.stats()
    per_mode = st["stored_m2l"] * 2048 + 8 * _near_k_total(full)
    fb, lb = full.cache_bytes(), lean.cache_bytes()
    print(f"cache_bytes cached {fb}, lean {lb}; per mode {per_mode}")
    assert per_mode > 0 and fb[0] == (2 * ks - 1) * per_mode
    assert lb[0] == 0
    assert lb[1] > 0 and lb[1] == fb[1]
    # a new setCoeff leaves the old operators allocated; cache_block frees them
    full.setCoeff(*rough_coeffs(full.getNodes(), 3))
    assert full.cache_bytes()[0] == fb[0]
    full.cache_block()
    assert full.cache_bytes() == (0, fb[1])
    # cache(id) after cache_block: that one mode resident again
    full.cache(2)
    assert full.cache_bytes()[0] == per_mode


def test_lean_shards_compose_to_the_unsharded_cached_result():
    """test_block_matvec_tree_order_and_shards_compose with every shard handle made
    ready by cache_block() only: tree-order input, owned slices out, three shards one
    after another, <= 1e-14 of the unsharded cached handle."""
    torch = _torch()
    import aniso_amd

    sz, d, ks = 24, 2, 3
    full = aniso_amd.Aniso(sz, d, ks, G, 8, 4, 20)
    coef = rough_coeffs(full.getNodes(), 5)
    full.setCoeff(*coef)
    for m in range(2 * ks - 1):
        full.cache(m)
    perm = torch.tensor(full.tree_perm(), device="cuda", dtype=torch.int64)
    U = torch.tensor(_input(ks, full.N, 3), device="cuda")
    ref = _matvec(full, U)
    Ut = U[:, perm].contiguous()
    parts = []
    for r in range(3):
        sh = aniso_amd.Aniso(sz, d, ks, G, 8, 4, 20)
        sh.set_shard(r, 3)
        sh.setCoeff(*coef)
        sh.cache_block()
        assert sh.cache_bytes()[0] == 0 and sh.cache_bytes()[1] > 0
        b, e = sh.shard()
        part = torch.zeros(ks, e - b, dtype=torch.float64, device="cuda")
        sh.block_op_dev(2, Ut, part, tree=True)
        torch.cuda.synchronize()
        parts.append(part)
    got = torch.cat(parts, 1)
    err = float(torch.linalg.norm(got - ref[:, perm]) / torch.linalg.norm(ref))
    print(f"lean shards vs unsharded cached: {err:.3e}")
    assert err <= 1e-14, err


def test_lean_shards_run_the_two_phase_and_the_one_call_forms():
    """The sharded entry points on lean handles: block_op_begin_dev / _end_dev around a
    hand-made root all-gather (three shards one after another) compose to the unsharded
    cached result, <= 1e-14; and a loopback communicator attaches to a lean handle
    (comm_init refuses a rank whose caches are not ready) and runs the one-call form."""
    torch = _torch()
    import aniso_amd

    sz, ks, world = 64, 5, 3
    full = aniso_amd.Aniso(sz, 1, ks, G, 10, 4, 20)
    coef = rough_coeffs(full.getNodes(), 6)
    full.setCoeff(*coef)
    for m in range(2 * ks - 1):
        full.cache(m)
    X = torch.tensor(_input(ks, full.N, 4), device="cuda")
    ref = torch.zeros_like(X)
    full.block_op_dev(2, X, ref, tree=True)
    torch.cuda.synchronize()
    hs = [aniso_amd.Aniso(sz, 1, ks, G, 10, 4, 20) for _ in range(world)]
    sends, outs, info = [], [], []
    for r, h in enumerate(hs):
        h.set_shard(r, world)
        h.setCoeff(*coef)
        h.cache_block()
        b, e = h.shard()
        ex = h.shard_exchange(ks)
        xr = torch.full_like(X, float("nan"))
        xr[:, b:e] = X[:, b:e]
        for lo, hi in h.shard_halo():
            xr[:, lo:hi] = X[:, lo:hi]
        y = torch.zeros(ks, max(e - b, 1), dtype=torch.float64, device="cuda")
        rs = torch.zeros(max(ex["root_chunk"] * ex["root_record"], 1), dtype=torch.float64, device="cuda")
        h.block_op_begin_dev(2, xr, y, rs)
        sends.append(rs[: ex["root_chunk"] * ex["root_record"]])
        outs.append(y)
        info.append((xr, b, e))
    recv = torch.cat(sends)
    Y = torch.zeros_like(X)
    for h, y, (xr, b, e) in zip(hs, outs, info):
        h.block_op_end_dev(2, xr, y, recv, world)
        Y[:, b:e] = y[:, : e - b]
    torch.cuda.synchronize()
    err = float(torch.linalg.norm(Y - ref) / torch.linalg.norm(ref))
    print(f"lean two-phase shards vs unsharded cached: {err:.3e}")
    assert err <= 1e-14, err
    assert all(h.cache_bytes()[0] == 0 for h in hs)
    # the one-call form on a loopback communicator: one rank's schedule, lean against cached
    lean = hs[1]
    cached = aniso_amd.Aniso(sz, 1, ks, G, 10, 4, 20)
    cached.set_shard(1, world)
    cached.setCoeff(*coef)
    for m in range(2 * ks - 1):
        cached.cache(m)
    # (the loopback leaves the other ranks' data out, so the values are not the
    # operator's: what is checked is that comm_init accepts a lean handle and that the
    # matvec takes the route it takes on a cached one)
    routes = []
    for h in (lean, cached):
        h.comm_init_loopback()
        h.block_op_sharded_dev(2, X.clone(), torch.zeros_like(X))
        h.sync()
        st = h.stats()
        routes.append((st["one_exchange_applies"], st["upper_partial_applies"]))
    print(f"one-call sharded matvec routes (lean, cached): {routes}")
    assert routes[0] == routes[1]
    assert lean.cache_bytes()[0] == 0


def test_cache_block_is_invalid_without_the_mode_shared_caches():
    """ANISO_HARMONIC=0: the block operator streams the per-mode operators, so
    cache_block is ANISO_ERR_INVALID (a child process: the switch is read at create)."""
    _torch()
    code = (
        "import sys\n"
        f"sys.path.insert(0, {ROOT!r})\n"
        "import numpy as np, aniso_amd\n"
        "a = aniso_amd.Aniso(8, 1, 5, 0.8, 6, 4, 20)\n"
        "xy = a.getNodes()\n"
        "a.setCoeff(1.0 + xy[:, 0], 1.5 + xy[:, 0])\n"
        "try:\n"
        "    a.cache_block()\n"
        "except aniso_amd.AnisoError as e:\n"
        "    print('code', e.code, 'harmonic' if 'ANISO_HARMONIC' in str(e) else '')\n"
        "    sys.exit(0)\n"
        "sys.exit(5)\n"
    )
    env = dict(os.environ, ANISO_HARMONIC="0")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert "code 1 harmonic" in r.stdout, r.stdout
