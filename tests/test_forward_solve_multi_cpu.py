"""The multi-source forward solve, the part that needs no device:
aniso_forward_solve_multi_dev and aniso_forward_solve_multi are public, exported and
wrapped, and every argument and state error returns its code with a message before the
device is touched (fake non-null device pointers where the check comes first)."""
import ctypes

import numpy as np
import pytest

import aniso_amd

NAMES = ("aniso_forward_solve_multi_dev", "aniso_forward_solve_multi")
INVALID, STATE = 1, 3
FAKE = ctypes.c_void_p(4096)  # a non-null "device pointer" no check may follow


def _handle(np_, ks=2):
    return aniso_amd.Aniso(8, 1, ks, 0.5, 6, np_, 20)


def _status(code):
    """(code, message) of a raw C call."""
    buf = ctypes.create_string_buffer(4096)
    aniso_amd.lib().aniso_last_error(buf, len(buf))
    return code, buf.value.decode(errors="replace")


def _other(N):
    return ctypes.c_void_p(4096 + 64 * N * 8)


def _dev(a, nrhs, q, ldq, x, ldx, restart=80, tol=1e-12, maxit=5, iters=True, src=1):
    it = (ctypes.c_int * max(nrhs, 1))() if iters else None
    return _status(aniso_amd.lib().aniso_forward_solve_multi_dev(a.address, nrhs, q, ldq, src, x, ldx, restart, tol, maxit,
                                                                 it, None, None, 0, None))


def _host(a, Q, k, X, restart=80, tol=1e-12, maxit=5, iters=True):
    dp = ctypes.POINTER(ctypes.c_double)
    q = Q.ctypes.data_as(dp) if Q is not None else None
    x = X.ctypes.data_as(dp) if X is not None else None
    it = (ctypes.c_int * max(k, 1))() if iters else None
    return _status(aniso_amd.lib().aniso_forward_solve_multi(a.address, q, k, 1, x, restart, tol, maxit, it, None))


def test_both_entries_are_exported_public_and_wrapped():
    public = aniso_amd.exported_symbols(public_only=True)
    lib = aniso_amd.lib()
    for name in NAMES:
        assert name in public, name
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    for m in ("forward_solve_multi_dev", "forward_solve_multi"):
        assert callable(getattr(aniso_amd.Aniso, m)), m


@pytest.mark.parametrize("np_", [4, 6])
def test_argument_errors_come_before_the_device(np_):
    a = _handle(np_)
    N = a.N
    other = _other(N)
    for kw in [dict(nrhs=-1, q=FAKE, ldq=N, x=other, ldx=N),               # nrhs < 0
               dict(nrhs=2, q=FAKE, ldq=N - 1, x=other, ldx=N),            # ldq below N
               dict(nrhs=2, q=FAKE, ldq=N, x=other, ldx=N - 1),            # ldx below N
               dict(nrhs=0, q=None, ldq=N - 1, x=None, ldx=N),             # ... also with nothing to do
               dict(nrhs=2, q=None, ldq=N, x=other, ldx=N),                # null q
               dict(nrhs=2, q=FAKE, ldq=N, x=None, ldx=N),                 # null x
               dict(nrhs=2, q=FAKE, ldq=N, x=other, ldx=N, iters=False),   # null iters
               dict(nrhs=2, q=FAKE, ldq=N, x=other, ldx=N, restart=0),
               dict(nrhs=2, q=FAKE, ldq=N, x=other, ldx=N, restart=401),
               dict(nrhs=2, q=FAKE, ldq=N, x=other, ldx=N, tol=0.0),
               dict(nrhs=2, q=FAKE, ldq=N, x=other, ldx=N, tol=-1e-3),
               dict(nrhs=2, q=FAKE, ldq=N, x=other, ldx=N, tol=float("nan")),
               dict(nrhs=2, q=FAKE, ldq=N, x=other, ldx=N, maxit=-1)]:
        code, msg = _dev(a, **kw)
        assert code == INVALID and msg, (kw, code, msg)
    for src in (0, 1):  # q and x overlap (the last row of q reaches into x)
        code, msg = _dev(a, 2, FAKE, N, ctypes.c_void_p(4096 + 8 * N), N, src=src)
        assert code == INVALID and "overlap" in msg, (code, msg)
    Q = np.zeros((N, 2), order="F")
    X = np.zeros((N, 2), order="F")
    assert _host(a, Q, -1, X)[0] == INVALID
    assert _host(a, None, 2, X)[0] == INVALID
    assert _host(a, Q, 2, None)[0] == INVALID
    assert _host(a, Q, 2, X, iters=False)[0] == INVALID
    assert _host(a, Q, 2, X, restart=0)[0] == INVALID
    assert _host(a, Q, 2, X, restart=401)[0] == INVALID
    assert _host(a, Q, 2, X, tol=0.0)[0] == INVALID
    assert _host(a, Q, 2, X, maxit=-1)[0] == INVALID
    code, msg = _host(a, Q, 2, Q)
    assert code == INVALID and "overlap" in msg, (code, msg)


@pytest.mark.parametrize("np_", [4, 6])
def test_no_columns_is_ok_and_touches_nothing(np_):
    a = _handle(np_)
    assert _dev(a, 0, None, a.N, None, a.N)[0] == 0
    assert _dev(a, 0, FAKE, a.N + 3, FAKE, a.N, iters=False)[0] == 0
    assert _host(a, None, 0, None)[0] == 0
    X, iters, relres = a.forward_solve_multi(np.zeros((a.N, 0)))
    assert X.shape == (a.N, 0) and iters.shape == (0,) and relres.shape == (0,)


@pytest.mark.parametrize("np_", [4, 6])
def test_before_set_coeff_is_a_state_error_that_names_aniso_cache(np_):
    a = _handle(np_)
    N = a.N
    for code, msg in (_dev(a, 3, FAKE, N, _other(N), N), _dev(a, 3, FAKE, N, _other(N), N, src=0),
                      _host(a, np.zeros((N, 3), order="F"), 3, np.zeros((N, 3), order="F"))):
        assert code == STATE, (code, msg)
        assert "aniso_set_coeff" in msg and "aniso_cache" in msg, msg


def test_a_sharded_handle_is_a_state_error():
    a = _handle(4)
    a.set_shard(0, 2)
    N = a.N
    for code, msg in (_dev(a, 2, FAKE, N, _other(N), N),
                      _host(a, np.zeros((N, 2), order="F"), 2, np.zeros((N, 2), order="F"))):
        assert code == STATE and "sharded" in msg, (code, msg)
    assert _dev(a, 0, None, N, None, N)[0] == 0  # nothing to do is still nothing to do


def test_python_wrappers_check_their_arrays_first():
    a = _handle(6)
    with pytest.raises(aniso_amd.AnisoError) as e:
        a.forward_solve_multi(np.zeros((a.N + 1, 2)))
    assert e.value.code == INVALID
    with pytest.raises(aniso_amd.AnisoError) as e:
        a.forward_solve_multi(np.zeros((a.N, 2)), x0=np.zeros((a.N, 3)))
    assert e.value.code == INVALID
    with pytest.raises(aniso_amd.AnisoError) as e:
        a.forward_solve_multi_dev(np.zeros((2, a.N)), np.zeros((2, a.N)))
    assert e.value.code == INVALID
