"""The block operator and its solve for several sources, the part that
needs no device: aniso_block_op_multi(_dev) and aniso_block_solve_multi(_dev) are public,
exported and wrapped, and every argument and state error returns its code with a message
before the device is touched (fake non-null device pointers where the check comes first)."""
import ctypes

import numpy as np
import pytest

import aniso_amd

NAMES = ("aniso_block_op_multi_dev", "aniso_block_op_multi", "aniso_block_solve_multi_dev", "aniso_block_solve_multi")
WRAPPERS = ("block_op_multi_dev", "block_op_multi", "block_solve_multi_dev", "block_solve_multi")
INVALID, STATE = 1, 3
KS = 2
FAKE = ctypes.c_void_p(4096)  # a non-null "device pointer" no check may follow
DP = ctypes.POINTER(ctypes.c_double)


def _handle(np_, ks=KS):
    return aniso_amd.Aniso(8, 1, ks, 0.5, 6, np_, 20)


def _status(code):
    """(code, message) of a raw C call."""
    buf = ctypes.create_string_buffer(4096)
    aniso_amd.lib().aniso_last_error(buf, len(buf))
    return code, buf.value.decode(errors="replace")


def _other(N):
    return ctypes.c_void_p(4096 + 64 * N * 8)  # far behind the rows FAKE starts


def _op(a, nsrc, x, ldx, out, ldo, which=2):
    return _status(aniso_amd.lib().aniso_block_op_multi_dev(a.address, which, nsrc, x, ldx, out, ldo, None))


def _op_host(a, U, nsrc, Out, which=2):
    u = U.ctypes.data_as(DP) if U is not None else None
    o = Out.ctypes.data_as(DP) if Out is not None else None
    return _status(aniso_amd.lib().aniso_block_op_multi(a.address, which, u, nsrc, o))


def _solve(a, nsrc, q, ldq, x, ldx, restart=60, tol=1e-11, maxit=5, iters=True, charge=1):
    it = (ctypes.c_int * max(nsrc, 1))() if iters else None
    return _status(aniso_amd.lib().aniso_block_solve_multi_dev(a.address, nsrc, q, ldq, charge, x, ldx, restart, tol,
                                                               maxit, it, None, None, 0, None))


def _solve_host(a, Q, nsrc, X, restart=60, tol=1e-11, maxit=5, iters=True):
    q = Q.ctypes.data_as(DP) if Q is not None else None
    x = X.ctypes.data_as(DP) if X is not None else None
    it = (ctypes.c_int * max(nsrc, 1))() if iters else None
    return _status(aniso_amd.lib().aniso_block_solve_multi(a.address, q, nsrc, 1, x, restart, tol, maxit, it, None))


def test_the_four_entries_are_exported_public_and_wrapped():
    public = aniso_amd.exported_symbols(public_only=True)
    lib = aniso_amd.lib()
    for name in NAMES:
        assert name in public, name
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    for m in WRAPPERS:
        assert callable(getattr(aniso_amd.Aniso, m)), m


@pytest.mark.parametrize("np_", [4, 6])
def test_operator_argument_errors_come_before_the_device(np_):
    a = _handle(np_)
    N = a.N
    other = _other(N)
    for kw in [dict(nsrc=-1, x=FAKE, ldx=N, out=other, ldo=N),            # nsrc < 0
               dict(nsrc=2, x=FAKE, ldx=N - 1, out=other, ldo=N),         # ldx below N
               dict(nsrc=2, x=FAKE, ldx=N, out=other, ldo=N - 1),         # ldo below N
               dict(nsrc=0, x=None, ldx=N - 1, out=None, ldo=N),          # ... also with nothing to do
               dict(nsrc=2, x=None, ldx=N, out=other, ldo=N),             # null x
               dict(nsrc=2, x=FAKE, ldx=N, out=None, ldo=N),              # null out
               dict(nsrc=2, x=FAKE, ldx=N, out=other, ldo=N, which=3),    # a bad which
               dict(nsrc=2, x=FAKE, ldx=N, out=other, ldo=N, which=-1),
               dict(nsrc=0, x=None, ldx=N, out=None, ldo=N, which=3)]:
        code, msg = _op(a, **kw)
        assert code == INVALID and msg, (kw, code, msg)
    # the last of the nsrc * ks input rows reaches into the output rows
    for which in (0, 1, 2):
        code, msg = _op(a, 2, FAKE, N, ctypes.c_void_p(4096 + 8 * N * (2 * KS - 1)), N, which=which)
        assert code == INVALID and "overlap" in msg, (code, msg)
    U = np.zeros((KS * N, 2), order="F")
    Out = np.zeros((KS * N, 2), order="F")
    assert _op_host(a, U, -1, Out)[0] == INVALID
    assert _op_host(a, None, 2, Out)[0] == INVALID
    assert _op_host(a, U, 2, None)[0] == INVALID
    assert _op_host(a, U, 2, Out, which=5)[0] == INVALID
    code, msg = _op_host(a, U, 2, U)
    assert code == INVALID and "overlap" in msg, (code, msg)


@pytest.mark.parametrize("np_", [4, 6])
def test_solve_argument_errors_come_before_the_device(np_):
    a = _handle(np_)
    N = a.N
    other = _other(N)
    for kw in [dict(nsrc=-1, q=FAKE, ldq=N, x=other, ldx=N),
               dict(nsrc=2, q=FAKE, ldq=N - 1, x=other, ldx=N),
               dict(nsrc=2, q=FAKE, ldq=N, x=other, ldx=N - 1),
               dict(nsrc=0, q=None, ldq=N - 1, x=None, ldx=N),
               dict(nsrc=2, q=None, ldq=N, x=other, ldx=N),
               dict(nsrc=2, q=FAKE, ldq=N, x=None, ldx=N),
               dict(nsrc=2, q=FAKE, ldq=N, x=other, ldx=N, iters=False),
               dict(nsrc=2, q=FAKE, ldq=N, x=other, ldx=N, restart=0),
               dict(nsrc=2, q=FAKE, ldq=N, x=other, ldx=N, restart=401),
               dict(nsrc=2, q=FAKE, ldq=N, x=other, ldx=N, tol=0.0),
               dict(nsrc=2, q=FAKE, ldq=N, x=other, ldx=N, tol=-1e-3),
               dict(nsrc=2, q=FAKE, ldq=N, x=other, ldx=N, tol=float("nan")),
               dict(nsrc=2, q=FAKE, ldq=N, x=other, ldx=N, maxit=-1)]:
        code, msg = _solve(a, **kw)
        assert code == INVALID and msg, (kw, code, msg)
    for charge in (0, 1):
        code, msg = _solve(a, 2, FAKE, N, ctypes.c_void_p(4096 + 8 * N * (2 * KS - 1)), N, charge=charge)
        assert code == INVALID and "overlap" in msg, (code, msg)
    Q = np.zeros((KS * N, 2), order="F")
    X = np.zeros((KS * N, 2), order="F")
    assert _solve_host(a, Q, -1, X)[0] == INVALID
    assert _solve_host(a, None, 2, X)[0] == INVALID
    assert _solve_host(a, Q, 2, None)[0] == INVALID
    assert _solve_host(a, Q, 2, X, iters=False)[0] == INVALID
    assert _solve_host(a, Q, 2, X, restart=0)[0] == INVALID
    assert _solve_host(a, Q, 2, X, restart=401)[0] == INVALID
    assert _solve_host(a, Q, 2, X, tol=0.0)[0] == INVALID
    assert _solve_host(a, Q, 2, X, maxit=-1)[0] == INVALID
    code, msg = _solve_host(a, Q, 2, Q)
    assert code == INVALID and "overlap" in msg, (code, msg)


@pytest.mark.parametrize("np_", [4, 6])
def test_no_sources_is_ok_and_touches_nothing(np_):
    a = _handle(np_)
    N = a.N
    for which in (0, 1, 2):
        assert _op(a, 0, None, N, None, N, which=which)[0] == 0
    assert _op(a, 0, FAKE, N + 3, FAKE, N)[0] == 0
    assert _op_host(a, None, 0, None)[0] == 0
    assert _solve(a, 0, None, N, None, N)[0] == 0
    assert _solve(a, 0, FAKE, N + 3, FAKE, N, iters=False)[0] == 0
    assert _solve_host(a, None, 0, None)[0] == 0
    assert a.block_op_multi(2, np.zeros((KS * N, 0))).shape == (KS * N, 0)
    X, iters, relres = a.block_solve_multi(np.zeros((KS * N, 0)))
    assert X.shape == (KS * N, 0) and iters.shape == (0,) and relres.shape == (0,)


@pytest.mark.parametrize("np_", [4, 6])
def test_before_set_coeff_is_a_state_error_that_names_aniso_cache_block(np_):
    a = _handle(np_)
    N = a.N
    z = lambda: np.zeros((KS * N, 3), order="F")  # noqa: E731
    for code, msg in (_op(a, 3, FAKE, N, _other(N), N), _op(a, 3, FAKE, N, _other(N), N, which=0),
                      _op_host(a, z(), 3, z()), _solve(a, 3, FAKE, N, _other(N), N),
                      _solve(a, 3, FAKE, N, _other(N), N, charge=0), _solve_host(a, z(), 3, z())):
        assert code == STATE, (code, msg)
        assert "aniso_set_coeff" in msg and "aniso_cache_block" in msg, msg


def test_a_sharded_handle_is_a_state_error():
    a = _handle(4)
    a.set_shard(0, 2)
    N = a.N
    z = lambda: np.zeros((KS * N, 2), order="F")  # noqa: E731
    for code, msg in (_op(a, 2, FAKE, N, _other(N), N), _op_host(a, z(), 2, z()),
                      _solve(a, 2, FAKE, N, _other(N), N), _solve_host(a, z(), 2, z())):
        assert code == STATE and "sharded" in msg, (code, msg)
    assert _op(a, 0, None, N, None, N)[0] == 0  # nothing to do is still nothing to do
    assert _solve(a, 0, None, N, None, N)[0] == 0


def test_python_wrappers_check_their_arrays_first():
    a = _handle(6)
    rows = KS * a.N
    with pytest.raises(aniso_amd.AnisoError) as e:
        a.block_op_multi(2, np.zeros((rows + 1, 2)))
    assert e.value.code == INVALID
    with pytest.raises(aniso_amd.AnisoError) as e:
        a.block_solve_multi(np.zeros((rows + 1, 2)))
    assert e.value.code == INVALID
    with pytest.raises(aniso_amd.AnisoError) as e:
        a.block_solve_multi(np.zeros((rows, 2)), x0=np.zeros((rows, 3)))
    assert e.value.code == INVALID
    with pytest.raises(aniso_amd.AnisoError) as e:
        a.block_op_multi_dev(2, np.zeros((2 * KS, a.N)), np.zeros((2 * KS, a.N)))
    assert e.value.code == INVALID
    with pytest.raises(aniso_amd.AnisoError) as e:
        a.block_solve_multi_dev(np.zeros((2 * KS, a.N)), np.zeros((2 * KS, a.N)))
    assert e.value.code == INVALID
