"""One mode on several vectors, the part that needs no device:
aniso_mapping_multi_dev, aniso_forward_multi_dev and aniso_mapping_multi are public and
exported, and every argument and state error returns its code with a message before the
device is touched (null device pointers where the check comes first)."""
import ctypes

import numpy as np
import pytest

import aniso_amd

NAMES = ("aniso_mapping_multi_dev", "aniso_forward_multi_dev", "aniso_mapping_multi")
INVALID, STATE, RANGE = 1, 3, 4
FAKE = ctypes.c_void_p(4096)  # a non-null "device pointer" no check may follow


def _handle(np_, ks=2):
    return aniso_amd.Aniso(8, 1, ks, 0.5, 6, np_, 20)


def _status(code):
    """(code, message) of a raw C call."""
    buf = ctypes.create_string_buffer(4096)
    aniso_amd.lib().aniso_last_error(buf, len(buf))
    return code, buf.value.decode(errors="replace")


def _map(a, id_, nrhs, x, ldx, out, ldo):
    return _status(aniso_amd.lib().aniso_mapping_multi_dev(a.address, id_, nrhs, x, ldx, out, ldo, None))


def _fwd(a, nrhs, x, ldx, out, ldo):
    return _status(aniso_amd.lib().aniso_forward_multi_dev(a.address, nrhs, x, ldx, out, ldo, None))


def _host(a, Q, k, id_, Out):
    dp = ctypes.POINTER(ctypes.c_double)
    q = Q.ctypes.data_as(dp) if Q is not None else None
    o = Out.ctypes.data_as(dp) if Out is not None else None
    return _status(aniso_amd.lib().aniso_mapping_multi(a.address, q, k, id_, o))


def test_the_three_entries_are_exported_and_public():
    public = aniso_amd.exported_symbols(public_only=True)
    lib = aniso_amd.lib()
    for name in NAMES:
        assert name in public, name
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    for m in ("mapping_multi_dev", "forward_multi_dev", "mapping_multi"):
        assert callable(getattr(aniso_amd.Aniso, m)), m


@pytest.mark.parametrize("np_", [4, 6])
def test_argument_errors_come_before_the_device(np_):
    a = _handle(np_)
    N = a.N
    other = ctypes.c_void_p(4096 + 64 * N * 8)
    for call in (lambda *r: _map(a, 0, *r), lambda *r: _fwd(a, *r)):
        for args in [(-1, FAKE, N, other, N),       # nrhs < 0
                     (2, FAKE, N - 1, other, N),    # ldx below N
                     (2, FAKE, N, other, N - 1),    # ldo below N
                     (0, None, N - 1, None, N),     # ... also with nothing to do
                     (2, None, N, other, N),        # null x
                     (2, FAKE, N, None, N)]:        # null out
            code, msg = call(*args)
            assert code == INVALID and msg, (args, code, msg)
    for id_ in (-1, 2 * a.ks - 1, 99):
        code, msg = _map(a, id_, 2, FAKE, N, other, N)
        assert code == RANGE and "out of range" in msg, (id_, code, msg)
    # x and out overlap: only the forward form reads x after out is stored
    code, msg = _fwd(a, 2, FAKE, N, ctypes.c_void_p(4096 + 8 * N), N)
    assert code == INVALID and "overlap" in msg, (code, msg)
    Q = np.zeros((N, 2), order="F")
    assert _host(a, Q, -1, 0, Q.copy(order="F"))[0] == INVALID
    assert _host(a, None, 2, 0, Q)[0] == INVALID
    assert _host(a, Q, 2, 0, None)[0] == INVALID
    assert _host(a, Q, 2, 2 * a.ks - 1, Q.copy(order="F"))[0] == RANGE


@pytest.mark.parametrize("np_", [4, 6])
def test_no_columns_is_ok_and_touches_nothing(np_):
    a = _handle(np_)
    assert _map(a, 0, 0, None, a.N, None, a.N)[0] == 0
    assert _map(a, 2, 0, FAKE, a.N + 3, FAKE, a.N)[0] == 0
    assert _fwd(a, 0, None, a.N, None, a.N)[0] == 0
    assert _host(a, None, 0, 0, None)[0] == 0
    assert a.mapping_multi(np.zeros((a.N, 0)), 1).shape == (a.N, 0)


@pytest.mark.parametrize("np_", [4, 6])
def test_before_set_coeff_is_a_state_error_that_names_aniso_cache(np_):
    a = _handle(np_)
    N = a.N
    other = ctypes.c_void_p(4096 + 64 * N * 8)
    for code, msg in (_map(a, 1, 3, FAKE, N, other, N), _fwd(a, 3, FAKE, N, other, N),
                      _host(a, np.zeros((N, 3), order="F"), 3, 1, np.zeros((N, 3), order="F"))):
        assert code == STATE, (code, msg)
        assert "aniso_set_coeff" in msg and "aniso_cache" in msg, msg


def test_a_sharded_handle_is_a_state_error():
    a = _handle(4)
    a.set_shard(0, 2)
    N = a.N
    other = ctypes.c_void_p(4096 + 64 * N * 8)
    for code, msg in (_map(a, 0, 2, FAKE, N, other, N), _fwd(a, 2, FAKE, N, other, N),
                      _host(a, np.zeros((N, 2), order="F"), 2, 0, np.zeros((N, 2), order="F"))):
        assert code == STATE and "sharded" in msg, (code, msg)
    assert _map(a, 0, 0, None, N, None, N)[0] == 0  # nothing to do is still nothing to do


def test_python_wrappers_check_their_tensors_first():
    a = _handle(6)
    with pytest.raises(aniso_amd.AnisoError) as e:
        a.mapping_multi(np.zeros((a.N + 1, 2)), 0)
    assert e.value.code == INVALID
    with pytest.raises(aniso_amd.AnisoError) as e:
        a.mapping_multi_dev(np.zeros((2, a.N)), 0, np.zeros((2, a.N)))
    assert e.value.code == INVALID
    with pytest.raises(aniso_amd.AnisoError) as e:
        a.forward_multi_dev(np.zeros((2, a.N)), np.zeros((2, a.N)))
    assert e.value.code == INVALID
