"""The general mixed-precision solve (aniso_solve_mixed_dev): the
16-column fp32 Arnoldi past the 48 rows its sweeps hold in registers, on an operator
the test supplies (aniso_arnoldi16_*), bit-identity with aniso_solve16_mixed_dev below
that limit, and the solve at the reference's restart 80 and at the cap 400 on a thick,
strongly scattering medium (sigma_s = 30, sigma_t = 30.01), where an inner cycle needs
more than 48 steps."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS32 = 2.0 ** -24


def _torch():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


@pytest.fixture(scope="module")
def thick():
    """sz = 64, d = 1 (N = 4,096), sigma_s = 30, sigma_t = 30.01, 20 config-5 sources."""
    torch = _torch()
    import aniso_amd
    from aniso_amd.solve import config5_charges, rhs_block

    a = aniso_amd.Aniso(64, 1, 1, 0.8, 10, 4, 20)
    xy = a.getNodes()
    a.setCoeff(np.full(a.N, 30.0), np.full(a.N, 30.01))
    a.cache(0)
    Q = np.stack([config5_charges(xy, s) for s in range(20)])
    B = rhs_block(a, torch.tensor(Q, device="cuda"))
    torch.cuda.synchronize()
    return a, Q, B


# ---- 1. the sweeps on a synthetic operator
M_SYN, N_SYN, ZERO_COL = 100, 2048, 6


def _synthetic():
    u = np.linspace(0.0, 1.0, N_SYN)
    kappa = 400.0 + 40.0 * np.arange(16)
    d = (1.0 + (kappa[None, :] - 1.0) * (u * u)[:, None]).astype(np.float32)  # (n, 16): column c multiplies by d[:, c]
    r = np.random.default_rng(5).standard_normal((N_SYN, 16)).astype(np.float32)
    r[:, ZERO_COL] = 0.0
    return d, r


def _run_arnoldi16(a, d, r):
    """begin, M_SYN steps with w = fp32(d * V[j]), the solution over all steps.  Returns
    the rows (m + 1, n, 16) fp32, the status after every step (m, 16, 4), the begin
    status (16, 4), x (n, 16) fp64 and the state blocks (16, total)."""
    torch = _torch()
    m, n16 = M_SYN, 16 * N_SYN
    dt = torch.tensor(d, device="cuda").reshape(-1)
    rt = torch.tensor(r, device="cuda", dtype=torch.float64).reshape(-1)
    rn = np.linalg.norm(r.astype(np.float64), axis=0)
    scale = torch.tensor(np.where(rn > 0.0, rn, 1.0), device="cuda")
    V = torch.full((m + 1, n16), float("nan"), dtype=torch.float32, device="cuda")
    state, part = a.arnoldi16_work(m)
    status = torch.zeros(64, dtype=torch.float64, device="cuda")
    hist = torch.zeros(m, 64, dtype=torch.float64, device="cuda")
    w = torch.empty(n16, dtype=torch.float32, device="cuda")
    a.arnoldi16_begin(V, m, rt, scale, state, part, status)
    first = status.clone()
    for j in range(m):
        torch.mul(V[j], dt, out=w)
        a.arnoldi16_step(V, m, j, w, state, part, status)
        hist[j].copy_(status)
    x = torch.zeros(n16, dtype=torch.float64, device="cuda")
    a.arnoldi16_solution(V, m, m, state, x)
    torch.cuda.synchronize()
    return (V.reshape(m + 1, N_SYN, 16).cpu().numpy(), hist.reshape(m, 16, 4).cpu().numpy(),
            first.reshape(16, 4).cpu().numpy(), x.reshape(N_SYN, 16).cpu().numpy(),
            state.reshape(16, -1).cpu().numpy())


def _cgs2_gmres(dc, b, m):
    """fp64 GMRES with CGS2 on A = diag(dc): |g_{j+1}| / |b| and h(j + 1, j) of every step."""
    nb = np.linalg.norm(b)
    Qm = np.zeros((m + 1, b.size))
    Qm[0] = b / nb
    cs, sn, g = np.zeros(m), np.zeros(m), np.zeros(m + 1)
    g[0] = nb
    est, sub = np.zeros(m), np.zeros(m)
    for j in range(m):
        wv = dc * Qm[j]
        h = Qm[: j + 1] @ wv
        wv = wv - h @ Qm[: j + 1]
        h2 = Qm[: j + 1] @ wv
        wv = wv - h2 @ Qm[: j + 1]
        col = np.zeros(j + 2)
        col[: j + 1] = h + h2
        col[j + 1] = sub[j] = np.linalg.norm(wv)
        Qm[j + 1] = wv / col[j + 1]
        for k in range(j):
            t = cs[k] * col[k] + sn[k] * col[k + 1]
            col[k + 1] = -sn[k] * col[k] + cs[k] * col[k + 1]
            col[k] = t
        den = np.hypot(col[j], col[j + 1])
        cs[j], sn[j] = col[j] / den, col[j + 1] / den
        g[j + 1] = -sn[j] * g[j]
        g[j] = cs[j] * g[j]
        est[j] = abs(g[j + 1]) / nb
    return est, sub


def test_sweeps_past_48_rows_on_a_synthetic_operator(thick):
    """100 steps of the 16-column Arnoldi at n = 2,048 points, column c's operator
    diag(fp32(1 + (kappa_c - 1) u^2)), kappa_c = 400 + 40 c; column 6's residual is zero.

    The stored rows P are the projected directions, not normalised (arnoldi.hpp): the
    orthonormal basis is Q = P T with the state block's T.  So orthonormality is asked of
    both: the cosines of the stored rows, |P_j . P_k| / (|P_j| |P_k|) for j != k, and
    |Q^T Q - I|, each <= 8 x 2^-24 (rounding p to fp32 moves an inner product by at most
    2^-24 of the norms' product; a skipped or doubled row leaves 1e-2 and more).
    T is the code's own, and Q = P T stops at column m - 1, so the norms of the stored
    rows are also pinned from outside: row j + 1 is A q_j - Q h, whose norm is the
    Hessenberg entry h(j + 1, j) of the fp64 reference GMRES; they agree to the 1 % the
    estimates are held to.
    Measured on the MI355X (printed below): see DESIGN.md §3.14."""
    a = thick[0]
    d, r = _synthetic()
    P, hist, first, x, state = _run_arnoldi16(a, d, r)
    m = M_SYN
    M1 = m + 1
    cols = [c for c in range(16) if c != ZERO_COL]
    assert not np.isnan(P).any() and not np.isnan(hist).any() and not np.isnan(x).any() and not np.isnan(first).any()
    # the zero column stays exactly zero
    assert not P[:, :, ZERO_COL].any() and not x[:, ZERO_COL].any()
    assert (hist[:, ZERO_COL, 0] == 0.0).all() and first[ZERO_COL, 0] == 0.0
    assert (hist[:, :, 2] == np.arange(1, m + 1)[:, None]).all()
    worst = {"cos_le48": 0.0, "cos_gt48": 0.0, "q_le48": 0.0, "q_gt48": 0.0}
    est_err = norm_err = 0.0
    for c in cols:
        Pc = P[:, :, c].astype(np.float64)  # (m + 1, n)
        nrm = np.linalg.norm(Pc, axis=1)
        C = np.abs((Pc @ Pc.T) / np.outer(nrm, nrm) - np.eye(M1))
        T = np.triu(state[c, 2 * M1 * m: 2 * M1 * m + M1 * M1].reshape(M1, M1).T)  # column-major M1 x M1
        # column m of T belongs to a step m that was not taken: Q's columns 0 .. m - 1
        Qc = T[:m, :m].T @ Pc[:m]
        G = np.abs(Qc @ Qc.T - np.eye(m))
        worst["cos_le48"] = max(worst["cos_le48"], C[:49, :49].max())
        worst["cos_gt48"] = max(worst["cos_gt48"], C[49:, :].max())
        worst["q_le48"] = max(worst["q_le48"], G[:49, :49].max())
        worst["q_gt48"] = max(worst["q_gt48"], G[49:, :].max())
        ref, sub = _cgs2_gmres(d[:, c].astype(np.float64), r[:, c].astype(np.float64), m)
        norm_err = max(norm_err, float(np.abs(nrm[1:] / sub - 1.0).max()))
        est_err = max(est_err, float(np.abs(hist[:, c, 0] / ref - 1.0).max()))
    last = hist[m - 1, :, 0]
    dd, rr = d.astype(np.float64), r.astype(np.float64)
    true = np.linalg.norm(rr - dd * x, axis=0) / np.where(np.linalg.norm(rr, axis=0) > 0, np.linalg.norm(rr, axis=0), 1.0)
    ratio = true[cols] / last[cols]
    print("arnoldi16 synthetic:", {k: float(v) for k, v in worst.items()}, "estimate error", est_err, "row norm error", norm_err,
          "estimates", float(hist[:, cols, 0].min()), float(hist[:, cols, 0].max()),
          "true / estimate", float(ratio.min()), float(ratio.max()))
    for k, v in worst.items():
        assert v <= 8 * EPS32, (k, v)
    assert est_err <= 0.01, est_err
    assert norm_err <= 0.01, norm_err
    assert (ratio <= 2.0).all() and (ratio >= 0.5).all(), ratio
    # repeatability: bitwise
    P2, hist2, first2, x2, state2 = _run_arnoldi16(a, d, r)
    assert np.array_equal(P, P2) and np.array_equal(hist, hist2) and np.array_equal(first, first2)
    assert np.array_equal(x, x2)


# ---- 2. bit-identity below the limit
def test_general_entry_is_bit_identical_to_the_16_row_entry_at_m_40():
    torch = _torch()
    import aniso_amd
    from aniso_amd.solve import config5_charges, rhs_block
    from conftest import main_coeffs

    a = aniso_amd.Aniso(64, 1, 1, 0.8, 10, 4, 20)
    xy = a.getNodes()
    a.setCoeff(*main_coeffs(xy))
    a.cache(0)
    Q = np.stack([config5_charges(xy, s) for s in range(16)])
    B = rhs_block(a, torch.tensor(Q, device="cuda"))
    X16, Xg = torch.zeros_like(B), torch.zeros_like(B)
    o16, i16, r16 = a.solve16_mixed_dev(B, X16, m=40)
    og, ig, lc, rg = a.solve_mixed_dev(B, Xg, m=40)
    torch.cuda.synchronize()
    assert (r16 <= 1e-12).all() and i16 > 0
    assert torch.equal(X16, Xg)
    assert (o16, i16) == (og, ig) and np.array_equal(r16, rg)
    assert 1 <= lc <= 40


# ---- 3. the solve past 48 rows
def test_solve_at_restart_80_on_a_thick_medium(thick):
    """20 sources (one full group, one padded) at m = 80: an inner cycle passes 48 steps
    (the oracle's fp64 GMRES needs 59-67 to 1e-6), every column reaches 1e-12, checked
    with the test's own fp64 residual on forward_block (<= 2e-12: that operator differs
    from the fp64 MFMA operator at rounding level).  Against the fp64 device GMRES the
    bound is 10 x the difference of two such solves at restarts 80 and 100 (the largest
    over the sources 0, 9, 19), measured here at run time; figures in DESIGN.md §3.14."""
    torch = _torch()
    from aniso_amd.solve import forward_block, gmres_mixed

    a, Q, B = thick
    X = torch.zeros_like(B)
    outer, inner, longest, rel = a.solve_mixed_dev(B, X, m=80, tol=1e-12, inner_tol=1e-6)
    torch.cuda.synchronize()
    W = torch.empty_like(B)
    forward_block(a, X, W)
    own = (torch.linalg.norm(B - W, dim=1) / torch.linalg.norm(B, dim=1)).cpu().numpy()
    print("restart 80:", dict(outer=outer, inner=inner, longest=longest, rel=float(rel.max()), own=float(own.max())))
    assert not torch.isnan(X).any()
    assert longest > 48, longest
    assert rel.shape == (20,) and (rel <= 1e-12).all(), rel
    assert (own <= 2e-12).all(), own
    Xd, od, idd, rd = gmres_mixed(a, B, m=80)
    assert torch.equal(Xd, X) and (od, idd) == (outer, inner) and np.array_equal(rd, rel)
    Xh = X.cpu().numpy()
    spread, diff = 0.0, 0.0
    for s in (0, 9, 19):
        it80, x80, _, _ = a.gmres(Q[s], m=80, maxit=400, tol=1e-12)
        it100, x100, _, _ = a.gmres(Q[s], m=100, maxit=400, tol=1e-12)
        assert it80 > 0 and it100 > 0
        spread = max(spread, float(np.linalg.norm(x80 - x100) / np.linalg.norm(x80)))
        diff = max(diff, float(np.linalg.norm(Xh[s] - x80) / np.linalg.norm(x80)))
    print("restart 80: fp64 solves at m = 80 / 100 differ by", spread, "; mixed against fp64", diff)
    assert diff <= 10.0 * spread, (diff, spread)


# ---- 4. restart 400 launches
def test_restart_400_launches_and_converges(thick):
    """m = 400 with one cycle per inner solve: the sweeps' and the small kernels' LDS at
    the cap (k16_update_wide and k16_axpy size theirs by the rows in use)."""
    torch = _torch()
    a, Q, B = thick
    B16 = B[:16].contiguous()
    X = torch.zeros_like(B16)
    outer, inner, longest, rel = a.solve_mixed_dev(B16, X, m=400, tol=1e-12, inner_tol=1e-6, max_cycles=1)
    torch.cuda.synchronize()
    print("restart 400:", dict(outer=outer, inner=inner, longest=longest, rel=float(rel.max())))
    assert not torch.isnan(X).any()
    assert 48 < longest <= 400, longest
    assert (rel <= 1e-12).all(), rel
    # the solve converges long before row 400: the last step of a 400-step cycle and the
    # solution over 400 steps launched directly, on a basis whose rows 1 .. 399 are zero
    m, n16 = 400, 16 * 512
    V = torch.zeros(m + 1, n16, dtype=torch.float32, device="cuda")
    V[m] = float("nan")
    state, part = a.arnoldi16_work(m)
    status = torch.zeros(64, dtype=torch.float64, device="cuda")
    r = torch.tensor(np.random.default_rng(7).standard_normal(n16), device="cuda")
    scale = torch.ones(16, dtype=torch.float64, device="cuda")
    a.arnoldi16_begin(V, m, r, scale, state, part, status)
    a.arnoldi16_step(V, m, m - 1, V[0].clone(), state, part, status)
    import aniso_amd

    with pytest.raises(aniso_amd.AnisoError) as e:  # w may not be the row the step writes
        a.arnoldi16_step(V, m, m - 2, V[m - 1], state, part, status)
    assert e.value.code == 1 and "overlaps" in str(e.value)
    x = torch.zeros(n16, dtype=torch.float64, device="cuda")
    a.arnoldi16_solution(V, m, m, state, x)
    torch.cuda.synchronize()
    assert torch.isfinite(V).all() and torch.isfinite(x).all() and torch.isfinite(status).all()
    assert (status.reshape(16, 4)[:, 2] == m).all()
