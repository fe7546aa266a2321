"""One mode on several vectors on the GPU: mapping_multi_dev,
forward_multi_dev and mapping_multi on high-order handles (np = 6, 8: the mode kernels of
mode_apply.hip on the mode-shared caches) against the CPU oracle at the same order and
against mapping on the same handle, column by column; on np = 4 handles, resident and
lean; and what the calls leave behind."""
import functools

import numpy as np
import pytest

from conftest import rough_coeffs

pytestmark = pytest.mark.gpu

TOL = 1e-10  # the suite's oracle-parity bound
G = 0.8
NCOL = 11    # 8 + 3: a full chunk and a padded one


def _torch():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def _rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def _coeffs(xy, coeffs):
    if coeffs == "demo":  # demo.m: sigma_s = 20, sigma_a = 0.2
        return 20.0 + 0.0 * xy[:, 0], 20.2 + 0.0 * xy[:, 0]
    return rough_coeffs(xy, 7)


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
def _oracle(sz, d, ks, ns, np_, coeffs, ml=20):
    from oracle.oracle_py import Oracle

    o = Oracle(sz, d, ks, G, ns, np_, ml)
    o.setCoeff(*_coeffs(o.getNodes(), coeffs))
    return o


@functools.lru_cache(maxsize=None)
def _oracle_mode(sz, d, ks, ns, np_, coeffs, ml, m):
    o = _oracle(sz, d, ks, ns, np_, coeffs, ml)
    o.cache(m)
    return o


@functools.lru_cache(maxsize=None)
def _columns(N, seed=11):
    X = np.random.default_rng(seed + N).uniform(-1.0, 1.0, (NCOL, N))
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def _oracle_column(shape, m, j):
    np_, sz, d, ks, ns, ml, coeffs = shape
    out = _oracle_mode(sz, d, ks, ns, np_, coeffs, ml, m).mapping(_columns(sz * sz * d * d)[j], m)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _mapping_column(shape, m, j):
    """a.mapping of column j: the handle's existing single-vector route."""
    np_, sz, d, ks, ns, ml, coeffs = shape
    out = _handle(sz, d, ks, ns, np_, coeffs, "block", ml).mapping(_columns(sz * sz * d * d)[j], m)
    out.setflags(write=False)
    return out


def _rows(torch, X, pad=7, extra=0, fill=float("nan")):
    """X's rows in a (rows + extra, N + pad) tensor filled with `fill`; returns the whole
    tensor and the view of the first rows."""
    k, N = X.shape
    t = torch.full((k + extra, N + pad), fill, dtype=torch.float64, device="cuda")
    t[:k, :N] = torch.tensor(X, device="cuda")
    return t, t[:k]


# np, sz, d, ks, ns, maxLevel, coefficients
SHAPES = [
    (6, 32, 1, 3, 10, 20, "demo"),   # N 1024: uniform tree, depth 3, 16-point leaves
    (6, 19, 3, 2, 8, 20, "rough"),   # N 3249: W and X lists (20 each), depth 4, leaves of 9..36 points
    (6, 20, 2, 2, 8, 2, "rough"),    # N 1600: depth capped, 100-point leaves (second staging chunk, 25 row quads)
    (8, 11, 3, 2, 8, 20, "rough"),   # N 1089: W and X lists (60 each), leaves of 12..64 points
    (8, 32, 1, 3, 10, 20, "demo"),   # N 1024: 64-point leaves, depth 2
]
_ID = lambda s: f"np{s[0]}sz{s[1]}d{s[2]}ks{s[3]}ml{s[5]}" if isinstance(s, tuple) else str(s)  # noqa: E731


# ---- 1. oracle parity

@pytest.mark.parametrize("nrhs", [1, 3, 5, 8, 11])
@pytest.mark.parametrize("shape", SHAPES, ids=_ID)
def test_every_column_matches_the_oracle_and_mapping(shape, nrhs):
    """Modes 0 (sigma_t diagonal), 1 (odd: the sign under transposed stored blocks) and
    2ks - 2 (longest recurrence); nrhs = 1, 3 (padded to 2, 4), 5, 8 and 11 = 8 + 3.  Rows
    of stride N + 7 with NaN in the gaps.  Every column: relative l2 <= 1e-10 against the
    oracle at the same order and <= 1e-12 against mapping on the same handle (both device
    routes lie within 2e-14 of the oracle; 1e-12 leaves 25x over their sum).  The gaps stay
    NaN and the rows of the output tensor past nrhs stay as they were."""
    torch = _torch()
    np_, sz, d, ks, ns, ml, coeffs = shape
    a = _handle(sz, d, ks, ns, np_, coeffs, "block", ml)
    N = a.N
    assert a.cache_bytes()[0] == 0
    cols = _columns(N)[:nrhs]
    for m in (0, 1, 2 * ks - 2):
        _, X = _rows(torch, cols)
        whole, Out = _rows(torch, np.zeros((nrhs, N)), extra=2)
        whole[nrhs:] = 7.0
        a.mapping_multi_dev(X, m, Out)
        torch.cuda.synchronize()
        got = whole.cpu().numpy()
        assert np.all(np.isnan(got[:nrhs, N:])), m          # the gaps are untouched
        assert np.all(got[nrhs:] == 7.0), m                 # and so are the rows past nrhs
        assert np.all(np.isnan(X.cpu().numpy()[:, N:])) and np.array_equal(X.cpu().numpy()[:, :N], cols)
        for j in range(nrhs):
            eo = _rel(got[j, :N], _oracle_column(shape, m, j))
            em = _rel(got[j, :N], _mapping_column(shape, m, j))
            print(f"np {np_} sz {sz} d {d} ml {ml} mode {m} nrhs {nrhs} column {j}: vs oracle {eo:.3e}, vs mapping {em:.3e}")
            assert eo <= TOL, (m, j, eo)
            assert em <= 1e-12, (m, j, em)


# ---- 2. columns are independent

@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[3]], ids=_ID)
def test_columns_are_independent_and_calls_repeat_bitwise(shape):
    """Column j of an 8-column call against the 1-column call on the same vector: <= 1e-13;
    two identical calls return equal bits."""
    torch = _torch()
    np_, sz, d, ks, ns, ml, coeffs = shape
    a = _handle(sz, d, ks, ns, np_, coeffs, "block", ml)
    N = a.N
    X = torch.tensor(_columns(N)[:8], device="cuda")
    for m in (1, 2 * ks - 2):
        out8 = torch.zeros(8, N, dtype=torch.float64, device="cuda")
        again = torch.ones(8, N, dtype=torch.float64, device="cuda")
        a.mapping_multi_dev(X, m, out8)
        a.mapping_multi_dev(X, m, again)
        torch.cuda.synchronize()
        assert torch.equal(out8, again), m
        for j in range(8):
            one = torch.zeros(1, N, dtype=torch.float64, device="cuda")
            a.mapping_multi_dev(X[j:j + 1], m, one)
            torch.cuda.synchronize()
            err = _rel(out8[j].cpu().numpy(), one[0].cpu().numpy())
            assert err <= 1e-13, (m, j, err)


# ---- 3. the forward form

def test_forward_multi_is_x_minus_mapping_of_sigma_s_x():
    """forward_multi_dev at nrhs = 3 on the np = 6, ks = 3 handle against x - mapping(sigma_s
    x, 0): largest difference <= 1e-13 x the largest |K_0(sigma_s x)| (the bound of
    test_forward_operator_and_gmres_match_reference); against the oracle, 1e-10."""
    torch = _torch()
    shape = SHAPES[0]
    np_, sz, d, ks, ns, ml, coeffs = shape
    a = _handle(sz, d, ks, ns, np_, coeffs, "block", ml)
    N = a.N
    ss, _ = _coeffs(a.getNodes(), coeffs)
    cols = _columns(N)[:3]
    _, X = _rows(torch, cols)
    whole, Out = _rows(torch, np.zeros((3, N)))
    a.forward_multi_dev(X, Out)
    torch.cuda.synchronize()
    got = whole.cpu().numpy()
    assert np.all(np.isnan(got[:, N:]))
    o = _oracle_mode(sz, d, ks, ns, np_, coeffs, ml, 0)
    for j in range(3):
        k0 = a.mapping(ss * cols[j], 0)
        scale = np.abs(k0).max()
        diff = np.abs(got[j, :N] - (cols[j] - k0)).max()
        odiff = np.abs(got[j, :N] - (cols[j] - o.mapping(ss * cols[j], 0))).max()
        print(f"forward column {j}: vs x - mapping {diff / scale:.3e}, vs the oracle {odiff / scale:.3e} (of max |K_0|)")
        assert diff <= 1e-13 * scale, (j, diff, scale)
        assert odiff <= TOL * scale, (j, odiff, scale)


# ---- 4. the host entry

@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[4]], ids=_ID)
def test_host_entry_equals_the_device_entry(shape):
    torch = _torch()
    np_, sz, d, ks, ns, ml, coeffs = shape
    a = _handle(sz, d, ks, ns, np_, coeffs, "block", ml)
    cols = _columns(a.N)[:3]
    for m in (0, 1):
        host = a.mapping_multi(cols.T, m)  # N x 3
        assert host.shape == (a.N, 3)
        out = torch.zeros(3, a.N, dtype=torch.float64, device="cuda")
        a.mapping_multi_dev(torch.tensor(cols, device="cuda"), m, out)
        torch.cuda.synchronize()
        assert np.array_equal(host.T, out.cpu().numpy()), m


# ---- 5. np = 4: a resident and a lean handle

@pytest.mark.parametrize("nrhs", [3, 9])
@pytest.mark.parametrize("how", ["modes", "block"])
def test_order_4_resident_and_lean(how, nrhs):
    """np = 4, (10, 2, ks = 2, ns = 8, rough): the resident handle (aniso_cache(id)) runs the
    batched apply, the lean one (aniso_cache_block) a pass per column; modes 0 and 2, every
    column <= 1e-13 from mapping on the same handle; the forward form likewise."""
    torch = _torch()
    sz, d, ks, ns = 10, 2, 2, 8
    a = _handle(sz, d, ks, ns, 4, "rough", how)
    N = a.N
    assert (a.cache_bytes()[0] == 0) == (how == "block")
    cols = _columns(N)[:nrhs]
    X = torch.tensor(cols, device="cuda")
    for m in (0, 2):
        out = torch.zeros(nrhs, N, dtype=torch.float64, device="cuda")
        a.mapping_multi_dev(X, m, out)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        for j in range(nrhs):
            err = _rel(got[j], a.mapping(cols[j], m))
            assert err <= 1e-13, (how, m, j, err)
    ss, _ = _coeffs(a.getNodes(), "rough")
    out = torch.zeros(nrhs, N, dtype=torch.float64, device="cuda")
    a.forward_multi_dev(X, out)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    for j in range(nrhs):
        k0 = a.mapping(ss * cols[j], 0)
        assert np.abs(got[j] - (cols[j] - k0)).max() <= 1e-13 * np.abs(k0).max(), (how, j)


# ---- 6. state is left as found; 7. the old names still refuse

def test_block_path_is_untouched_and_old_names_still_refuse():
    """On the np = 6, ks = 5, sz = 32 handle of test_repeatable_and_refusing: block_op(2, U),
    mapping_multi_dev at nrhs = 8 (it grows the work buffers it shares with the block path),
    block_op(2, U): equal bits, no per-mode cache.  mapping_batched and forward_dev still
    return ANISO_ERR_STATE there."""
    torch = _torch()
    import aniso_amd

    sz, d, ks, ns, np_ = 32, 1, 5, 10, 6
    a = _handle(sz, d, ks, ns, np_, "demo")
    N = a.N
    U = np.random.default_rng(5).uniform(-1.0, 1.0, (ks, N))
    first = a.block_op(2, U)
    out = torch.zeros(8, N, dtype=torch.float64, device="cuda")
    a.mapping_multi_dev(torch.tensor(_columns(N)[:8], device="cuda"), 3, out)
    torch.cuda.synchronize()
    assert np.isfinite(out.cpu().numpy()).all()
    assert np.array_equal(a.block_op(2, U), first)
    assert a.cache_bytes()[0] == 0
    q = torch.zeros(N, dtype=torch.float64, device="cuda")
    for name, call in (("mapping_batched", lambda: a.mapping_batched(np.ones((N, 2)), 0)),
                       ("forward_dev", lambda: a.forward_dev(q, torch.zeros_like(q)))):
        with pytest.raises(aniso_amd.AnisoError) as e:
            call()
        assert e.value.code == 3, (name, e.value.code, str(e.value))
        assert "high-order" in str(e.value), (name, str(e.value))
    assert np.array_equal(a.block_op(2, U), first)
