"""What one apply leaves behind on its handle: nothing.  A block matvec with the fused
subtraction, a pass of the ks > 8 operator, a lean mapping and a sharded matvec each
describe themselves to the batched apply for one call only (ApplyCall, aniso_op.hpp);
a call that raises half-way, or simply returns, must not change what the next call on
the same handle computes.  Every comparison is bitwise against a fresh handle on a
route with a fixed summation order."""
import ctypes

import numpy as np
import pytest

from conftest import rough_coeffs
from test_gpu_sharded_passes import _CountingCollectives, _Shared, _handle, _run_ranks

pytestmark = pytest.mark.gpu

G, NP, ML = 0.8, 4, 20


def _torch():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def _make(sz, ks, ns, coef=None, lean=False):
    import aniso_amd

    a = aniso_amd.Aniso(sz, 1, ks, G, ns, NP, ML)
    if coef is None:
        coef = rough_coeffs(a.getNodes(), 3)
    a.coef = coef
    a.setCoeff(*coef)
    if lean:
        a.cache_block()
    else:
        for m in range(2 * ks - 1):
            a.cache(m)
    return a


def _raw(fn, *args):
    """A C ABI call past the Python wrapper's shape checks: the library's own refusal."""
    import aniso_amd

    code = fn(*args)
    if code != 0:
        aniso_amd._check(code)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream(torch):
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _block_op(a, which, U):
    torch = _torch()
    out = torch.zeros_like(U)
    a.block_op_dev(which, U, out)
    torch.cuda.synchronize()
    return out


def _mapping(a, q, m):
    torch = _torch()
    out = torch.zeros_like(q)
    a.mapping_dev(q, m, out)
    torch.cuda.synchronize()
    return out


def test_no_leak_after_a_matvec_that_raises():
    """sz 12, ks 5, ns 8 (the smallest shape with a down pass: the subtraction is fused
    into it): block_op_dev(2) with an output stride below N raises inside the apply;
    mapping_dev(q, 0) and block_op_dev(1) on the same handle afterwards are bitwise a
    fresh handle's (deterministic sums on both).  A subtraction left behind would
    subtract the input from them."""
    torch = _torch()
    import aniso_amd

    a = _make(12, 5, 8)
    fresh = _make(12, 5, 8, a.coef)
    a.set_deterministic(1)
    fresh.set_deterministic(1)
    N = a.N
    rng = np.random.default_rng(21)
    U = torch.tensor(rng.uniform(-1, 1, (5, N)), device="cuda")
    q = torch.tensor(rng.uniform(-1, 1, N), device="cuda")
    out = torch.zeros_like(U)
    with pytest.raises(aniso_amd.AnisoError) as e:
        _raw(aniso_amd.lib().aniso_block_op_dev, a.address, 2, _ptr(U), N, _ptr(out), N - 1, 0, _stream(torch))
    assert e.value.code == 1 and "leading dimension" in str(e.value), str(e.value)
    torch.cuda.synchronize()
    assert float(out.abs().max()) == 0.0  # refused before anything was launched
    got_m, ref_m = _mapping(a, q, 0), _mapping(fresh, q, 0)
    assert float(ref_m.abs().max()) > 0 and torch.equal(got_m, ref_m)
    got_b, ref_b = _block_op(a, 1, U), _block_op(fresh, 1, U)
    assert float(ref_b.abs().max()) > 0 and torch.equal(got_b, ref_b)
    # and the matvec itself still subtracts
    assert torch.equal(_block_op(a, 2, U), _block_op(fresh, 2, U))


@pytest.fixture(scope="module")
def ks9():
    """sz 16, ks 9 lean: a handle the calls under test have run on, a fresh one, the
    input and the fresh handle's block_op_dev(1) (the passes sum in a fixed order)."""
    torch = _torch()
    used = _make(16, 9, 8, lean=True)
    fresh = _make(16, 9, 8, used.coef, lean=True)
    U = torch.tensor(np.random.default_rng(22).uniform(-1, 1, (9, used.N)), device="cuda")
    ref = _block_op(fresh, 1, U)
    assert torch.isfinite(ref).all() and float(ref.abs().max()) > 0
    return used, U, ref


def test_no_leak_after_a_pass(ks9):
    """block_pass_dev(0, 1, 0), then two passes that raise (chunk index out of range,
    output stride below N): the full block_op_dev(1) stays bitwise the fresh handle's."""
    torch = _torch()
    import aniso_amd

    a, U, ref = ks9
    N = a.N
    out8 = torch.zeros(8, N, dtype=torch.float64, device="cuda")
    a.block_pass_dev(0, 1, 0, U, out8)
    torch.cuda.synchronize()
    assert float(out8[0].abs().max()) > 0
    assert torch.equal(_block_op(a, 1, U), ref)
    fn = aniso_amd.lib().aniso_block_pass_dev
    for I, ldo, what in ((2, N, "chunk index"), (1, N - 1, "leading dimension")):
        with pytest.raises(aniso_amd.AnisoError) as e:
            _raw(fn, a.address, 1, I, 0, _ptr(U), N, _ptr(out8), ldo, _stream(torch))
        assert e.value.code == 1 and what in str(e.value), str(e.value)
        assert torch.equal(_block_op(a, 1, U), ref), what


def test_no_leak_after_a_lean_mapping(ks9):
    """mapping_dev(q, 3) on a lean handle is one pass of the offset form; the block
    operator after it is bitwise a fresh handle's, at ks 9 and -- the deterministic
    matvec -- at ks 5."""
    torch = _torch()
    a, U, ref = ks9
    q = torch.tensor(np.random.default_rng(23).uniform(-1, 1, a.N), device="cuda")
    assert a.cache_bytes()[0] == 0  # no per-mode operators: the lean route
    assert float(_mapping(a, q, 3).abs().max()) > 0
    assert torch.equal(_block_op(a, 1, U), ref)
    b = _make(16, 5, 8, a.coef, lean=True)
    fresh = _make(16, 5, 8, a.coef, lean=True)
    b.set_deterministic(1)
    fresh.set_deterministic(1)
    assert float(_mapping(b, q, 3).abs().max()) > 0
    U5 = U[:5].contiguous()
    got, want = _block_op(b, 2, U5), _block_op(fresh, 2, U5)
    assert float(want.abs().max()) > 0 and torch.equal(got, want)


@pytest.mark.parametrize("ks", [10, 5])
def test_no_leak_after_a_refused_sharded_matvec(ks, monkeypatch):
    """Two thread-ranks at sz 32: set_coeff after comm_init without re-caching makes the
    sharded matvec raise on every rank before any collective; after cache_block() it
    agrees with the unsharded operator (<= 1e-13, the bound of
    tests/test_gpu_sharded_passes.py), and mapping_tree_dev on the same handle is
    bitwise a fresh shard's."""
    torch = _torch()
    import aniso_amd

    monkeypatch.setenv("ANISO_ONE_EXCHANGE", "1")
    sz, world = 32, 2
    full = _handle(sz, 1, ks, ML, None)
    coef, N = full.coef, full.N
    rng = np.random.default_rng(24 + ks)
    X = torch.tensor(rng.uniform(-1, 1, (ks, N)), device="cuda")
    q = torch.tensor(rng.uniform(-1, 1, N), device="cuda")
    ref = torch.zeros_like(X)
    full.block_op_dev(2, X, ref, tree=True)
    torch.cuda.synchronize()
    hs = [_handle(sz, 1, ks, ML, coef, r, world) for r in range(world)]
    shared = _Shared(world)
    colls = [_CountingCollectives(r, shared) for r in range(world)]
    outs, maps, refused = [None] * world, [None] * world, [None] * world

    def body(r):
        h = hs[r]
        h.comm_init_callbacks(colls[r].struct)
        b, e = h.shard()
        x = torch.full_like(X, float("nan"))
        x[:, b:e] = X[:, b:e]
        y = torch.zeros_like(X)
        h.setCoeff(*coef)  # the caches are gone, the communicator stays
        n0 = len(colls[r].calls)
        try:
            h.block_op_sharded_dev(2, x, y)
        except aniso_amd.AnisoError as ex:
            refused[r] = (ex.code != 0, len(colls[r].calls) - n0)
        h.cache_block()
        h.block_op_sharded_dev(2, x, y)
        h.sync()
        outs[r] = y[:, b:e].clone()
        h.cache(0)
        maps[r] = h.mapping_tree_dev(q, 0, torch.zeros(e - b, dtype=torch.float64, device="cuda")).clone()
        h.sync()

    _run_ranks(world, shared, body)
    assert refused == [(True, 0)] * world, refused
    Y = torch.cat(outs, dim=1)
    assert not torch.isnan(Y).any()
    err = float(torch.linalg.norm(Y - ref) / torch.linalg.norm(ref))
    print(f"ks={ks}: sharded matvec after a refusal, rel err vs unsharded {err:.3e}")
    assert err <= 1e-13, err
    for r in range(world):
        fresh = _handle(sz, 1, ks, ML, coef, r, world)
        fresh.cache(0)
        b, e = fresh.shard()
        want = fresh.mapping_tree_dev(q, 0, torch.zeros(e - b, dtype=torch.float64, device="cuda"))
        torch.cuda.synchronize()
        assert float(want.abs().max()) > 0 and torch.equal(maps[r], want), r
