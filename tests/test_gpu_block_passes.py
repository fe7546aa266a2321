"""The block operator beyond 8 Fourier blocks: ks > 8 runs as
ceil(ks / 8)^2 passes of the harmonic kernels' offset form over the mode-shared
caches.  Against the oracle's per-mode composition, against the generic per-mode
stream pass by pass, against single-mode device applies at a multi-tier size, through
the block solve, and the limits (sharded / deterministic handles)."""
import ctypes
import functools

import numpy as np
import pytest

from conftest import gaussian_charge, main_coeffs, rough_coeffs

pytestmark = pytest.mark.gpu

TOL = 1e-10


def _torch():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def _rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


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


@functools.lru_cache(maxsize=None)
def _case(sz, d, ks, ns, ml, coeffs):
    """A handle and an oracle on one geometry with every mode cached, and an input
    (built once per shape; the tests leave them as they found them)."""
    import aniso_amd
    from oracle.oracle_py import Oracle

    a = aniso_amd.Aniso(sz, d, ks, 0.8, ns, 4, ml)
    o = Oracle(sz, d, ks, 0.8, ns, 4, ml)
    xy = a.getNodes()
    ss, st = main_coeffs(xy) if coeffs == "main" else rough_coeffs(xy, 7)
    a.setCoeff(ss, st)
    o.setCoeff(ss, st)
    for m in range(2 * ks - 1):
        a.cache(m)
        o.cache(m)
    U = np.random.default_rng(sz + ks).uniform(-1, 1, (ks, a.N))
    U[0] += gaussian_charge(xy)
    U.setflags(write=False)
    return a, o, xy, ss, U


SHAPES = [
    # sz, d, ks, ns, maxLevel, coeffs
    (16, 1, 9, 8, 20, "main"),    # one padded chunk of 1
    (12, 1, 12, 8, 20, "rough"),
    (10, 2, 16, 8, 20, "rough"),  # two full chunks, d = 2 corrections
    (11, 1, 10, 6, 20, "rough"),  # odd sz: W / X lists
    (24, 1, 9, 10, 2, "rough"),   # 64-point leaves: the G = 64 near kernel
    (8, 1, 17, 8, 20, "main"),    # P = 3
]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda c: f"sz{c[0]}d{c[1]}ks{c[2]}ns{c[3]}ml{c[4]}{c[5]}")
def test_block_operator_beyond_8_blocks_matches_oracle(shape):
    """forward, mforward and x - mforward(x) on ks > 8 blocks (device and host entry
    points) against the oracle's per-mode composition, <= 1e-10; on the ks = 12 case
    also aniso_apply_block with a foreign sigma_s / g, and the handle's own afterwards."""
    torch = _torch()
    a, o, xy, ss, U = _case(*shape)
    ks = shape[2]
    assert a.stats()["harmonic"] == 1
    Ud = torch.tensor(U, device="cuda")
    for which in (0, 1, 2):
        out = torch.zeros_like(Ud)
        a.block_op_dev(which, Ud, out)
        torch.cuda.synchronize()
        ref = _block_ref(o, U, a.g, ss, which)
        err = _rel(out.cpu().numpy(), ref)
        print(f"ks={ks} which={which}: device rel err {err:.3e}")
        assert err <= TOL, (which, err)
        host = a.block_op(which, U.reshape(-1))
        assert _rel(host, ref) <= TOL, (which, _rel(host, ref))
    if ks == 12:
        ss2 = ss * 0.5 + 0.25
        ref = _block_ref(o, U, 0.6, ss2, 2)
        host = a.apply_block(U, ss2, 0.6)
        assert _rel(host, ref) <= TOL, _rel(host, ref)
        # ... and the handle's own sigma_s / g again afterwards (no state leaks)
        assert _rel(a.block_op(2, U), _block_ref(o, U, a.g, ss, 2)) <= TOL


@pytest.mark.parametrize("which", [0, 1])
def test_one_pass_matches_the_generic_stream(which):
    """Every pass (I, J) of the ks = 12 operator against aniso_apply_block_dev on the
    pass's zero-padded input chunk with its (23, 8, 8) sub-mix: 23 terms at 8
    right-hand sides are no harmonic structure, so that call streams the per-mode
    operators -- independent of the offset windows.  Tolerance: the harmonic-versus-
    stream comparison's (test_harmonic_block_apply_matches_per_mode_stream), 1e-13."""
    torch = _torch()
    import aniso_amd

    a, _, _, _, U = _case(12, 1, 12, 8, 20, "rough")
    ks, N = 12, a.N
    chunk, P = aniso_amd.block_pass_plan(ks)
    assert (chunk, P) == (8, 2)
    mix = aniso_amd.block_mixes(ks, a.g, which != 0)
    Ud = torch.tensor(U, device="cuda")
    for I in range(P):
        for J in range(P):
            i0, b0 = chunk * I, chunk * J
            ni, nb = min(chunk, ks - i0), min(chunk, ks - b0)
            sub = np.zeros((2 * ks - 1, chunk, chunk))
            sub[:, :ni, :nb] = mix[:, i0:i0 + ni, b0:b0 + nb]
            x8 = torch.zeros(chunk, N, dtype=torch.float64, device="cuda")
            x8[:nb] = Ud[b0:b0 + nb]
            ref = torch.zeros(chunk, N, dtype=torch.float64, device="cuda")
            a.apply_block_dev(x8, np.arange(2 * ks - 1), sub, ref, use_sigma=bool(which))
            got = torch.full((chunk, N), 7.0, dtype=torch.float64, device="cuda")
            a.block_pass_dev(which, I, J, Ud, got)
            torch.cuda.synchronize()
            err = float(torch.linalg.norm(got - ref) / torch.linalg.norm(ref))
            print(f"which={which} pass ({I}, {J}): rel err {err:.3e}")
            assert err <= 1e-13, (which, I, J, err)
            assert not got[ni:].any()  # the padded output rows are masked


def test_block_pass_arguments_are_checked():
    torch = _torch()
    import aniso_amd

    a, _, _, _, U = _case(12, 1, 12, 8, 20, "rough")
    Ud = torch.tensor(U, device="cuda")
    out = torch.zeros(8, a.N, dtype=torch.float64, device="cuda")
    for which, I, J in [(2, 0, 0), (0, 2, 0), (1, 0, -1)]:
        with pytest.raises(aniso_amd.AnisoError) as e:
            a.block_pass_dev(which, I, J, Ud, out)
        assert e.value.code == 1


def test_block_matvec_12_blocks_mid_size_matches_mode_applies():
    """N = 16,384 (a multi-tier tree, several clusters), ks = 12: x - mforward(x) equals
    its composition from single-mode device applies (1e-13, as
    test_block_matvec_at_config3_size_matches_mode_applies), repeats (1e-15), and
    tree-order I/O is the permuted original-order result (1e-14)."""
    torch = _torch()
    import aniso_amd

    ks, g = 12, 0.8
    a = aniso_amd.Aniso(128, 1, ks, g, 10, 4, 20)
    xy = a.getNodes()
    ss, st = main_coeffs(xy)
    a.setCoeff(ss, st)
    for m in range(2 * ks - 1):
        a.cache(m)
    U = torch.tensor(np.random.default_rng(9).uniform(-1, 1, (ks, a.N)), device="cuda")
    y1, y2 = torch.zeros_like(U), torch.zeros_like(U)
    a.block_op_dev(2, U, y1)
    a.block_op_dev(2, U, y2)
    sd = torch.tensor(ss, device="cuda")
    mix = aniso_amd.block_mixes(ks, g, True)
    ref = U.clone()
    tmp = torch.zeros(a.N, dtype=torch.float64, device="cuda")
    for m in range(2 * ks - 1):
        for b in range(ks):
            if not np.any(mix[m, :, b]):
                continue
            a.mapping_dev((U[b] * sd).contiguous(), m, tmp)
            for i in range(ks):
                if mix[m, i, b]:
                    ref[i] -= float(mix[m, i, b]) * tmp
    perm = torch.tensor(a.tree_perm(), device="cuda", dtype=torch.int64)
    Ut = U[:, perm].contiguous()
    yt = torch.zeros_like(U)
    a.block_op_dev(2, Ut, yt, tree=True)
    torch.cuda.synchronize()
    rep = float(torch.linalg.norm(y1 - y2) / torch.linalg.norm(y1))
    err = float(torch.linalg.norm(y1 - ref) / torch.linalg.norm(ref))
    tre = float(torch.linalg.norm(yt - y1[:, perm]) / torch.linalg.norm(y1))
    print(f"ks=12 N={a.N}: vs mode applies {err:.3e}, repeat {rep:.3e}, tree order {tre:.3e}")
    assert rep <= 1e-15
    assert err <= 1e-13
    assert tre <= 1e-14


def _gmres_matlab(apply, b, restart, tol, maxit):
    """Restarted GMRES with MATLAB's stopping rule (relative residual <= tol, checked
    per step on the estimate and confirmed explicitly at each cycle's end), modified
    Gram-Schmidt, numpy on the host: the reference solve of aniso.m:159-173 over the
    oracle's operator.  Returns (x, total steps, final relative residual)."""
    x = np.zeros_like(b)
    nb = np.linalg.norm(b)
    r = b - apply(x)
    beta = np.linalg.norm(r)
    total = 0
    for _ in range(maxit):
        if beta / nb <= tol:
            break
        V = np.zeros((restart + 1, b.size))
        H = np.zeros((restart + 1, restart))
        V[0] = r / beta
        g = np.zeros(restart + 1)
        g[0] = beta
        cs, sn = np.zeros(restart), np.zeros(restart)
        used = 0
        for i in range(restart):
            w = apply(V[i])
            for k in range(i + 1):
                H[k, i] = V[k] @ w
                w = w - H[k, i] * V[k]
            H[i + 1, i] = np.linalg.norm(w)
            V[i + 1] = w / H[i + 1, i]
            for k in range(i):
                t = cs[k] * H[k, i] + sn[k] * H[k + 1, i]
                H[k + 1, i] = -sn[k] * H[k, i] + cs[k] * H[k + 1, i]
                H[k, i] = t
            den = np.hypot(H[i, i], H[i + 1, i])
            cs[i], sn[i] = H[i, i] / den, H[i + 1, i] / den
            H[i, i], H[i + 1, i] = den, 0.0
            g[i + 1], g[i] = -sn[i] * g[i], cs[i] * g[i]
            total += 1
            used = i + 1
            if abs(g[i + 1]) / nb <= tol:
                break
        y = np.linalg.solve(np.triu(H[:used, :used]), g[:used])
        x = x + V[:used].T @ y
        r = b - apply(x)
        beta = np.linalg.norm(r)
    return x, total, beta / nb


def test_block_solve_10_blocks_matches_gmres_over_oracle():
    """aniso.m:159-173's solve at ks = 10: rhs = forward(charge), gmres(A, rhs, 400,
    1e-11, 400) through aniso_block_solve against the restated GMRES over the oracle's
    composition: the same step count, solutions within 1e-10; the device entry point
    from a nonzero guess converges to the same solution."""
    torch = _torch()
    a, o, xy, ss, _ = _case(12, 1, 10, 10, 20, "main")
    ks = 10
    charge = np.zeros((ks, a.N))
    charge[0] = gaussian_charge(xy)
    rhs = _block_ref(o, charge, a.g, ss, 0).reshape(-1)

    def A(v):
        return _block_ref(o, np.asarray(v, dtype=np.float64).reshape(ks, a.N), a.g, ss, 2).reshape(-1)

    tol = 1e-11
    xr, its_ref, rr_ref = _gmres_matlab(A, rhs, 400, tol, 400)
    its, u, hist, rr = a.block_solve(rhs, 400, tol, 400)
    assert its > 0 and rr <= tol and rr_ref <= tol
    assert its == its_ref, (its, its_ref)
    assert _rel(u.reshape(-1), xr) <= 1e-10, _rel(u.reshape(-1), xr)
    assert hist.size == its and hist[-1] <= tol
    rd = torch.tensor(rhs.reshape(ks, a.N), device="cuda")
    xd = torch.tensor(0.5 * xr.reshape(ks, a.N), device="cuda")
    its_d, _, rr_d = a.block_solve_dev(rd, xd, 400, tol, 400)
    assert its_d > 0 and rr_d <= tol
    assert _rel(xd.cpu().numpy().reshape(-1), xr) <= 1e-10


def test_sharded_and_deterministic_handles_refuse_more_than_8_blocks():
    torch = _torch()
    import aniso_amd

    a = aniso_amd.Aniso(16, 1, 9, 0.8, 8, 4, 20)
    with pytest.raises(aniso_amd.AnisoError) as e:
        a.set_deterministic(1)
    assert e.value.code == 1 and "8" in str(e.value)
    a.set_deterministic(0)  # switching it off is no error
    a.set_shard(0, 2)
    xy = a.getNodes()
    a.setCoeff(*main_coeffs(xy))
    x = torch.zeros(9, a.N, dtype=torch.float64, device="cuda")
    for tree in (False, True):
        out = torch.zeros(9, a.N if not tree else a.n_owned(), dtype=torch.float64, device="cuda")
        with pytest.raises(aniso_amd.AnisoError) as e:
            a.block_op_dev(0, x, out, tree=tree)
        assert e.value.code == 1 and "8" in str(e.value)
    with pytest.raises(aniso_amd.AnisoError) as e:
        a.block_op(0, np.zeros(9 * a.N))
    assert e.value.code == 1
    with pytest.raises(aniso_amd.AnisoError) as e:
        a.block_pass_dev(0, 0, 0, x, torch.zeros(8, a.N, dtype=torch.float64, device="cuda"))
    assert e.value.code == 1


@pytest.mark.parametrize("shape", [(12, 1, 8, 8, 20, "rough"), (12, 1, 5, 8, 20, "main")],
                         ids=lambda c: f"ks{c[2]}")
def test_up_to_8_blocks_are_untouched(shape):
    """ks <= 8: one pass, the stats keep their count, the block operator matches the
    oracle as before, and the one pass is the operator."""
    torch = _torch()
    import aniso_amd

    a, o, xy, ss, U = _case(*shape)
    ks = shape[2]
    assert aniso_amd.block_pass_plan(ks) == (ks, 1)
    full = np.zeros(40, dtype=np.int64)
    n = ctypes.c_int()
    P64 = ctypes.POINTER(ctypes.c_int64)
    assert aniso_amd.lib().aniso_stats_n(a.address, full.ctypes.data_as(P64), len(full), ctypes.byref(n)) == 0
    assert n.value == 34
    Ud = torch.tensor(U, device="cuda")
    for which in (0, 1, 2):
        out = torch.zeros_like(Ud)
        a.block_op_dev(which, Ud, out)
        torch.cuda.synchronize()
        ref = _block_ref(o, U, a.g, ss, which)
        assert _rel(out.cpu().numpy(), ref) <= TOL, (which, _rel(out.cpu().numpy(), ref))
        if which < 2:
            one = torch.zeros_like(Ud)
            a.block_pass_dev(which, 0, 0, Ud, one)
            torch.cuda.synchronize()
            assert torch.equal(one, out) or _rel(one.cpu().numpy(), out.cpu().numpy()) <= 1e-15
    a.set_deterministic(1)  # allowed up to 8 blocks
    a.set_deterministic(0)
