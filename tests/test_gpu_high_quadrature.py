"""Quadrature rules 4..6 (quadRule = d, the upper half of the range aniso_create
accepts) on the device against the CPU oracle: the k_corr<D,K> and k16_corr<T,D>
instances for D = 4, 5, 6, the runtime-d loops of the cache build and the line
integral, and the shard halo plan at d2 = 16 .. 36 points per square.

Tolerances are the suite's own (test_gpu_parity.py): 1e-10 against the oracle
(BASELINE.json north_star), per-stage errors relative to the full output's norm,
1e-12 mixed for the line integral, 1e-13 / 1e-14 between two fp64 device paths that
differ in summation order only, and the fp32 operator's 2e-6 / 2e-5.  The oracle's
cancellation ratio R = (sum of the stage norms) / (2 pi |total|) at these shapes is
1.5 .. 2.3 for mode 0 and up to 6.3 for mode 2; for the fp32 operator's apply it is
1.7 .. 2.2, below the 2.9 of test_fp32_mfma_operator_matches_fp64's (30, 3) case, so
no limit is rescaled.  Measured errors per path: DESIGN.md section 3.4.1.

Shapes are (sz, d, ns, maxLevel, coeffs); the block count ks comes with each test.
Every shape has 324 .. 1,296 points; S4, S5 and S6 are odd-sized or non-power-of-two
grids whose trees have W and X lists."""
import functools

import numpy as np
import pytest

from conftest import gaussian_charge, main_coeffs, rough_coeffs
from test_gpu_parity import TOL, _block_ref, _rel, _torch, _two_phase_shards

pytestmark = pytest.mark.gpu

G = 0.8
S4 = (9, 4, 8, 20, "rough")
S5 = (7, 5, 8, 20, "rough")
S6 = (6, 6, 8, 20, "rough")
S6M = (5, 6, 10, 20, "main")     # uniform tree, smooth coefficients
S6LEAF = (3, 6, 8, 1, "rough")   # 81-point leaves: a square's 36 points lie in four leaves
S6ONE = (1, 6, 8, 20, "main")    # one square: every dr / dc bound of the stencil is hit
S4K9 = (5, 4, 8, 20, "rough")    # ks = 9: the passes of a block operator of more than 8 blocks
S6K8 = (4, 6, 8, 20, "rough")


def _id(shape):
    return "sz%dd%dns%dml%d%s" % shape


def _coeffs(shape, xy):
    return main_coeffs(xy) if shape[4] == "main" else rough_coeffs(xy, shape[0])


def _new_handle(shape, ks):
    import aniso_amd

    sz, d, ns, ml, _ = shape
    a = aniso_amd.Aniso(sz, d, ks, G, ns, 4, ml)
    a.setCoeff(*_coeffs(shape, a.getNodes()))
    return a


@functools.lru_cache(maxsize=None)
def _oracle(shape, ks):
    """The oracle of a shape with every mode of ks blocks cached; shared, read only."""
    from oracle.oracle_py import Oracle

    sz, d, ns, ml, _ = shape
    o = Oracle(sz, d, ks, G, ns, 4, ml)
    xy = o.getNodes()
    ss, st = _coeffs(shape, xy)
    o.setCoeff(ss, st)
    for m in range(2 * ks - 1):
        o.cache(m)
    return o, xy, ss


@functools.lru_cache(maxsize=None)
def _cached(shape, ks):
    """A handle with cache(m) run for every mode; the tests that share it leave it as
    they found it."""
    a = _new_handle(shape, ks)
    for m in range(2 * ks - 1):
        a.cache(m)
    return a


def _ratio(st):
    """The oracle's cancellation ratio of one apply: stage norms over the total's."""
    return float(sum(np.linalg.norm(st[k]) for k in range(5)) / (2 * np.pi * np.linalg.norm(st[5])))


@pytest.mark.parametrize("shape", [S4, S5, S6, S6ONE], ids=_id)
def test_stages_match_oracle_high_d(shape):
    """Far + near field, stencil (nearRemoval + refineAddOn) and singular term of
    mapping_dev, each alone against oracle.mapping_stages, relative to the full
    output: a wrong stencil table, a wrong singular moment / Legendre shift table and
    a wrong cache show up in different masks.  Reaches k_corr<D,1> with each flag
    alone and the cache kernels' runtime-d line integral, D = 4, 5, 6."""
    import aniso_amd

    torch = _torch()
    a = _cached(shape, 2)
    o, xy, _ = _oracle(shape, 2)
    q = np.random.default_rng(5).uniform(-1, 1, a.N)
    qd = torch.tensor(q, device="cuda")
    s = 1.0 / (2 * np.pi)
    for m in (0, 1, 2):
        st = o.mapping_stages(q, m)
        for mask, ref in ((aniso_amd.STAGE_FAR | aniso_amd.STAGE_NEAR, (st[0] + st[1]) * s),
                          (aniso_amd.STAGE_STENCIL, (st[2] + st[3]) * s),
                          (aniso_amd.STAGE_SING, st[4] * s)):
            od = torch.zeros(a.N, dtype=torch.float64, device="cuda")
            a.mapping_dev(qd, m, od, mask=mask)
            torch.cuda.synchronize()
            err = float(np.linalg.norm(od.cpu().numpy() - ref) / np.linalg.norm(st[5]))
            print(f"stages {_id(shape)} mode {m} mask {mask}: err / |total| {err:.3e}, R {_ratio(st):.2f}")
            assert err <= TOL, (shape, m, mask, err)


@pytest.mark.parametrize("shape", [S4, S5, S6, S6M, S6LEAF, S6ONE], ids=_id)
def test_mapping_matches_oracle_high_d(shape):
    """The full single-mode apply, modes 0 .. 2, a random and the Gaussian charge:
    k_corr<D,1>, the M2L / near cache kernels and the line integral at d = 4, 5, 6;
    W / X lists, a uniform tree, 81-point leaves that split squares, one square."""
    _torch()
    a = _cached(shape, 2)
    o, xy, _ = _oracle(shape, 2)
    rng = np.random.default_rng(shape[0] * 31 + shape[1])
    for q in (rng.uniform(-1, 1, a.N), gaussian_charge(xy)):
        for m in (0, 1, 2):
            err = _rel(a.mapping(q, m), o.mapping(q, m))
            print(f"mapping {_id(shape)} mode {m}: rel err {err:.3e}")
            assert err <= TOL, (shape, m, err)


@pytest.mark.parametrize("d", [4, 5, 6])
def test_line_integrals_match_oracle_high_d(d):
    """sigma_piece / legendre_all with Px[kMaxD] filled to d = 4, 5, 6: vertical,
    horizontal, short, grid-corner and random segments against the oracle's
    recursive lineIntegral."""
    _torch()
    shape = (7, d, 8, 20, "rough")
    a = _new_handle(shape, 1)
    o, _, _ = _oracle(shape, 1)
    rng = np.random.default_rng(11 + d)
    seg = rng.uniform(0.001, 0.999, (1500, 4))
    seg[:200, 2] = seg[:200, 0]          # vertical segments
    seg[200:400, 3] = seg[200:400, 1]    # horizontal segments
    seg[400:500, 2:] = seg[400:500, :2] + 1e-3 * rng.uniform(-1, 1, (100, 2))  # short
    k = np.arange(1, 7) / 7.0            # through grid corners
    seg[500:506] = np.stack([k * 0 + 0.01, k * 0 + 0.01, k, k], 1)
    got = a.line_integrals(seg)
    ref = np.array([o.line_integral(*s) for s in seg])
    err = float(np.max(np.abs(got - ref) / np.maximum(1.0, np.abs(ref))))
    print(f"line integrals d={d}: max mixed err {err:.3e}")
    assert err <= 1e-12, err


@pytest.mark.parametrize("shape,ks", [(S4, 2), (S5, 3), (S6, 5), (S6K8, 8), (S4K9, 9)],
                         ids=lambda v: _id(v) if isinstance(v, tuple) else f"ks{v}")
def test_block_operator_matches_oracle_high_d(shape, ks):
    """aniso.m's forward, mforward and x - mforward(x) against the oracle's per-mode
    composition: k_corr<D,K> for K = 2, 4 (3 padded), 5, 8 at D = 4, 5, 6, and the
    ks = 9 passes (K = 8 windows) at D = 4."""
    torch = _torch()
    a = _cached(shape, ks)
    o, xy, ss = _oracle(shape, ks)
    U = np.random.default_rng(shape[0] + ks).uniform(-1, 1, (ks, a.N))
    U[0] += gaussian_charge(xy)
    Ud = torch.tensor(U, device="cuda")
    mf = _block_ref(o, U, G, ss, 1)
    for which, ref in ((0, _block_ref(o, U, G, ss, 0)), (1, mf), (2, U - mf)):
        out = torch.zeros_like(Ud)
        a.block_op_dev(which, Ud, out)
        torch.cuda.synchronize()
        err = _rel(out.cpu().numpy(), ref)
        print(f"block op {_id(shape)} ks={ks} which={which}: rel err {err:.3e}")
        assert err <= TOL, (which, err)


def test_apply_block_generic_mixes_high_d():
    """apply_block_dev on S5 (D = 5): arbitrary mixes of three mode terms, nrhs = 3
    (padded to k_corr<5,4>), strided input and output rows, with and without sigma_s;
    the columns past N stay untouched."""
    torch = _torch()
    a = _cached(S5, 3)
    o, xy, ss = _oracle(S5, 3)
    nrhs, ids = 3, [0, 3, 1]
    rng = np.random.default_rng(nrhs)
    X = rng.uniform(-1, 1, (nrhs, a.N))
    mixes = rng.uniform(-1, 1, (len(ids), nrhs, nrhs))
    xbuf = torch.zeros(nrhs, a.N + 13, dtype=torch.float64, device="cuda")
    xbuf[:, :a.N] = torch.tensor(X, device="cuda")
    for use_sigma in (False, True):
        obuf = torch.full((nrhs, a.N + 5), 7.0, dtype=torch.float64, device="cuda")
        a.apply_block_dev(xbuf[:, :a.N], ids, mixes, obuf[:, :a.N], use_sigma=use_sigma)
        torch.cuda.synchronize()
        base = [[o.mapping(X[b] * ss if use_sigma else X[b], m) for b in range(nrhs)] for m in ids]
        ref = np.zeros((nrhs, a.N))
        for t in range(len(ids)):
            for i in range(nrhs):
                for b in range(nrhs):
                    ref[i] += mixes[t, i, b] * base[t][b]
        got = obuf.cpu().numpy()
        err = _rel(got[:, :a.N], ref)
        print(f"apply_block S5 nrhs=3 sigma={use_sigma}: rel err {err:.3e}")
        assert err <= TOL, (use_sigma, err)
        assert np.all(got[:, a.N:] == 7.0)  # padding columns untouched


@pytest.mark.parametrize("shape", [S4, S6, S6ONE, S6LEAF], ids=_id)
def test_fp64_mfma_operator_high_d(shape):
    """The fp64 16-right-hand-side operator (k16_corr<double,D>, D = 4, 6): the forward
    operator and the mapping of modes 1 and 2 against the VALU path column by column
    (<= 1e-13: only the summation order differs), and mapping_batched for 11 and 16
    columns against the oracle.  S6leaf: the 16-column gather of a square that lies in
    four leaves."""
    torch = _torch()
    a = _cached(shape, 2)
    o, xy, _ = _oracle(shape, 2)
    rng = np.random.default_rng(shape[0] + shape[1])
    X = torch.tensor(rng.uniform(-1, 1, (a.N, 16)), device="cuda")
    Y = torch.zeros_like(X)
    a.forward16_f64_dev(X, Y)
    Xc = X.t().contiguous()
    ref = torch.zeros_like(Xc)
    for j in range(16):
        a.forward_tree_dev(Xc[j], ref[j])
    torch.cuda.synchronize()
    err = float(torch.linalg.norm(Y.t() - ref) / torch.linalg.norm(ref))
    print(f"fp64 mfma {_id(shape)} forward vs VALU: {err:.3e}")
    assert err <= 1e-13, err
    for m in (1, 2):
        a.mapping16_f64_dev(m, X, Y)
        for j in range(16):
            a.mapping_tree_dev(Xc[j], m, ref[j])
        torch.cuda.synchronize()
        err = float(torch.linalg.norm(Y.t() - ref) / torch.linalg.norm(ref))
        print(f"fp64 mfma {_id(shape)} mapping mode {m} vs VALU: {err:.3e}")
        assert err <= 1e-13, (m, err)
    for k, m in ((11, 1), (16, 0)):
        Q = rng.uniform(-1, 1, (a.N, k))
        B = a.mapping_batched(Q, m)
        for j in range(k):
            err = _rel(B[:, j], o.mapping(Q[:, j], m))
            assert err <= TOL, (k, m, j, err)
        print(f"fp64 mfma {_id(shape)} mapping_batched {k} columns mode {m}: last column rel err {err:.3e}")


@pytest.mark.parametrize("shape", [S4, S5, S6, S6ONE, S6LEAF], ids=_id)
def test_fp32_mfma_operator_high_d(shape):
    """Config 5's fp32 operator (k16_corr<float,D>, D = 4, 5, 6) against the fp64
    forward operator column by column, at the limits of
    test_fp32_mfma_operator_matches_fp64 (err <= 2e-6, the operator part alone
    kerr <= 2e-5).  The oracle's cancellation ratio R of column 0's apply goes into the
    assertion message: a miss at an R far above the d <= 3 cases' would be conditioning.
    Measured on the MI355X: err 3.6e-8 .. 6.5e-8, kerr 7.1e-8 .. 1.9e-7, R 1.7 .. 2.2
    (the oracle's R at the (30, 3) case is 2.9): the limits stand as they are."""
    torch = _torch()
    a = _new_handle(shape, 1)
    a.cache(0)
    rng = np.random.default_rng(shape[0] + shape[1])
    X = torch.tensor(rng.uniform(-1, 1, (a.N, 16)), device="cuda", dtype=torch.float32)
    Y = torch.zeros_like(X)
    a.forward_f32_dev(X, Y)
    Xd = X.double().t().contiguous()
    ref = torch.zeros_like(Xd)
    for j in range(16):
        a.forward_tree_dev(Xd[j], ref[j])
    torch.cuda.synchronize()
    err = float(torch.linalg.norm(Y.double().t() - ref) / torch.linalg.norm(ref))
    kerr = float(torch.linalg.norm((Xd - Y.double().t()) - (Xd - ref)) / torch.linalg.norm(Xd - ref))
    # R of the operator's apply K_0 (sigma_s x) for column 0 (tree order -> original order)
    o, _, ss = _oracle(shape, 1)
    x0 = np.zeros(a.N)
    x0[a.tree_perm()] = Xd[0].cpu().numpy()
    R = _ratio(o.mapping_stages(x0 * ss, 0))
    print(f"fp32 mfma {_id(shape)}: err {err:.3e} kerr {kerr:.3e} R {R:.2f}")
    assert err <= 2e-6 and kerr <= 2e-5, (shape, err, kerr, R)


def test_shards_compose_high_d():
    """S4 (16-point squares: the halo plan's 3 x 3 squares around each own target at
    d2 = 16), ks = 2, three ranks: every rank's two-phase block matvec on an input
    that is NaN outside its own range and halo, against the unsharded matvec."""
    torch = _torch()
    sz, d, ns, ml, _ = S4
    ks, world = 2, 3
    full = _cached(S4, ks)
    coef = _coeffs(S4, full.getNodes())
    X = torch.tensor(np.random.default_rng(sz).uniform(-1, 1, (ks, full.N)), device="cuda")
    ref = torch.zeros_like(X)
    full.block_op_dev(2, X, ref, tree=True)
    torch.cuda.synchronize()
    err, nans, halo = _two_phase_shards(sz, d, ks, ml, coef, world, X, ref, g=G, ns=ns)
    print(f"two-phase shards S4 world=3: rel err {err:.3e}, NaNs {nans}, halo / N {halo:.3f}")
    assert nans == 0
    assert halo > 0
    assert err <= 1e-13, err


def test_sharded_mapping_composes_high_d():
    """S5 (25-point squares), two ranks: each shard's single-mode apply writes its own
    targets only, and the two compose to the unsharded apply."""
    torch = _torch()
    import aniso_amd
    from aniso_amd import dist as adist

    sz, d, ns, ml, _ = S5
    full = _cached(S5, 2)
    coef = _coeffs(S5, full.getNodes())
    q = torch.tensor(np.random.default_rng(2).uniform(-1, 1, full.N), device="cuda")
    ref = torch.zeros_like(q)
    full.mapping_dev(q, 1, ref)
    ranges = adist.shard_ranges(full, 2)
    perm = torch.tensor(full.tree_perm(), device="cuda", dtype=torch.int64)
    got = torch.zeros_like(q)
    for r in range(2):
        sh = aniso_amd.Aniso(sz, d, 2, G, ns, 4, ml)
        sh.set_shard(r, 2)
        sh.setCoeff(*coef)
        sh.cache(1)
        out = torch.full_like(q, float("nan"))
        sh.mapping_dev(q, 1, out)
        own = perm[ranges[r][0]:ranges[r][1]]
        got[own] = out[own]
    torch.cuda.synchronize()
    err = float(torch.linalg.norm(got - ref) / torch.linalg.norm(ref))
    print(f"sharded mapping S5 world=2: rel err {err:.3e}")
    assert err <= 1e-14, err


def test_lean_handle_high_d():
    """S6, ks = 5 after cache_block() only: the block operator against the oracle, no
    per-mode operator held, and the bits of the cached handle's result with the
    deterministic sums on both (test_lean_equals_cached_on_the_clustered_launch's
    form of the comparison at ks <= 8)."""
    torch = _torch()
    ks = 5
    lean = _new_handle(S6, ks)
    lean.cache_block()
    full = _cached(S6, ks)
    o, xy, ss = _oracle(S6, ks)
    U = np.random.default_rng(17).uniform(-1, 1, (ks, lean.N))
    U[0] += gaussian_charge(xy)
    Ud = torch.tensor(U, device="cuda")
    out = torch.zeros_like(Ud)
    lean.block_op_dev(2, Ud, out)
    torch.cuda.synchronize()
    err = _rel(out.cpu().numpy(), _block_ref(o, U, G, ss, 2))
    print(f"lean S6 ks=5: rel err vs oracle {err:.3e}")
    assert err <= TOL, err
    assert lean.stats()["harmonic"] == 1 and lean.cache_bytes()[0] == 0
    outf = torch.zeros_like(Ud)
    full.block_op_dev(2, Ud, outf)
    torch.cuda.synchronize()
    errf = float(torch.linalg.norm(out - outf) / torch.linalg.norm(outf))
    print(f"lean S6 ks=5 vs cached, default sums: {errf:.3e}")
    assert errf <= 1e-14, errf
    lean.set_deterministic(1)
    full.set_deterministic(1)
    try:
        dl, df = torch.zeros_like(Ud), torch.zeros_like(Ud)
        lean.block_op_dev(2, Ud, dl)
        full.block_op_dev(2, Ud, df)
        torch.cuda.synchronize()
    finally:
        full.set_deterministic(0)
    assert float(torch.linalg.norm(dl)) > 0
    assert torch.equal(dl, df), float(torch.linalg.norm(dl - df) / torch.linalg.norm(df))
