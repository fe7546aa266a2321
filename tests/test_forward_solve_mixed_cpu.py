"""The reduced-precision route of a high-order handle, the part that needs
no device: the new entries are exported (public, or development for the pass list) with
argtypes and wrappers, and every argument error and refusal comes with its code before the
device is touched (null or fake device pointers)."""
import ctypes
import gc

import numpy as np
import pytest

import aniso_amd

INVALID, STATE, RANGE = 1, 3, 4
FAKE = ctypes.c_void_p(4096)  # a non-null "device pointer" no check may follow

PUBLIC = {"aniso_cache_f32": "cache_f32", "aniso_cache_f32_bytes": "cache_f32_bytes",
          "aniso_mapping_multi_f32_dev": "mapping_multi_f32_dev",
          "aniso_forward_multi_f32_dev": "forward_multi_f32_dev",
          "aniso_forward_solve_multi_mixed_dev": "forward_solve_multi_mixed_dev",
          "aniso_forward_solve_multi_mixed": "forward_solve_multi_mixed"}
DEV = {"aniso_forward_solve_mixed_calls": "forward_solve_mixed_calls"}


def _handle(np_=6, ks=2, shard=None):
    return aniso_amd.Aniso(8, 1, ks, 0.5, 6, np_, 20, shard=shard)


def _status(code):
    buf = ctypes.create_string_buffer(4096)
    aniso_amd.lib().aniso_last_error(buf, len(buf))
    return code, buf.value.decode(errors="replace")


def _mapping(h, id_, nrhs, x, ldx, out, ldo):
    return _status(aniso_amd.lib().aniso_mapping_multi_f32_dev(h.address, id_, nrhs, x, ldx, out, ldo, None))


def _forward(h, nrhs, x, ldx, out, ldo):
    return _status(aniso_amd.lib().aniso_forward_multi_f32_dev(h.address, nrhs, x, ldx, out, ldo, None))


def _solve(h, nrhs, q, ldq, x, ldx, restart=80, tol=1e-12, inner_tol=1e-4, maxit=5, max_outer=10, iters=True,
           outer=True):
    it = (ctypes.c_int * 16)() if iters else None
    ou = (ctypes.c_int * 16)() if outer else None
    return _status(aniso_amd.lib().aniso_forward_solve_multi_mixed_dev(
        h.address, nrhs, q, ldq, 1, x, ldx, restart, tol, inner_tol, maxit, max_outer, it, ou, None, None))


def test_the_new_entries_are_exported_with_argtypes_and_wrappers():
    every, public = aniso_amd.exported_symbols(), aniso_amd.exported_symbols(public_only=True)
    for name, wrapper in PUBLIC.items():
        assert name in public, name
        assert getattr(aniso_amd.lib(), name).argtypes is not None, name
        assert callable(getattr(aniso_amd.Aniso, wrapper)), wrapper
    for name, wrapper in DEV.items():
        assert name in every and name not in public, name
        assert getattr(aniso_amd.lib(), name).argtypes is not None, name
        assert callable(getattr(aniso_amd.Aniso, wrapper)), wrapper


def test_a_fresh_handle_has_no_mirrors_and_no_passes():
    a = _handle()
    assert a.cache_f32_bytes() == 0
    got = a.forward_solve_mixed_calls()
    assert got.shape == (0, 2) and got.dtype == np.int32
    assert aniso_amd.lib().aniso_cache_f32_bytes(a.address, None) == INVALID
    assert aniso_amd.lib().aniso_forward_solve_mixed_calls(a.address, None, 0, None) == INVALID


def test_argument_errors_of_the_f32_operator_entries():
    a = _handle()
    N = a.N
    other = ctypes.c_void_p(4096 + 64 * N * 8)
    for args in [(-1, FAKE, N, other, N), (2, FAKE, N - 1, other, N), (2, FAKE, N, other, N - 1),
                 (2, None, N, other, N), (2, FAKE, N, None, N)]:
        assert _mapping(a, 0, *args)[0] == INVALID, args
        assert _forward(a, *args)[0] == INVALID, args
    for id_ in (-1, 2 * a.ks - 1):
        code, msg = _mapping(a, id_, 2, FAKE, N, other, N)
        assert code == RANGE and "out of range" in msg, (id_, code, msg)
    code, msg = _forward(a, 2, FAKE, N, ctypes.c_void_p(4096 + 8 * N), N)
    assert code == INVALID and "overlap" in msg, (code, msg)
    assert _mapping(a, 0, 0, None, N, None, N)[0] == 0  # nothing to do
    assert a.mode_apply_calls().size == 0


def test_argument_errors_of_the_mixed_solve():
    a = _handle()
    N = a.N
    other = ctypes.c_void_p(4096 + 64 * N * 8)
    ok = (2, FAKE, N, other, N)
    for args in [(-1, FAKE, N, other, N), (2, FAKE, N - 1, other, N), (2, FAKE, N, other, N - 1),
                 (2, None, N, other, N), (2, FAKE, N, None, N)]:
        assert _solve(a, *args)[0] == INVALID, args
    code, msg = _solve(a, 2, FAKE, N, ctypes.c_void_p(4096 + 8 * N), N)
    assert code == INVALID and "overlap" in msg, (code, msg)
    for kw in [dict(restart=0), dict(restart=401), dict(tol=0.0), dict(tol=-1.0), dict(tol=float("nan")),
               dict(maxit=-1), dict(inner_tol=0.0), dict(inner_tol=1.0), dict(inner_tol=-0.5),
               dict(inner_tol=float("nan")), dict(max_outer=0), dict(max_outer=-3), dict(iters=False),
               dict(outer=False)]:
        code, msg = _solve(a, *ok, **kw)
        assert code == INVALID and msg, (kw, code, msg)
    assert _solve(a, 0, None, N, None, N)[0] == 0  # nothing to do
    assert a.forward_solve_mixed_calls().shape == (0, 2)
    Q = np.zeros((N, 3), order="F")
    for kw in (dict(inner_tol=2.0), dict(max_outer=0), dict(restart=0)):
        with pytest.raises(aniso_amd.AnisoError) as e:
            a.forward_solve_multi_mixed(Q, **kw)
        assert e.value.code == INVALID, kw


def test_order_4_is_refused_and_pointed_to_its_own_mixed_solve():
    a = _handle(np_=4)
    N = a.N
    other = ctypes.c_void_p(4096 + 64 * N * 8)
    for code, msg in (_mapping(a, 0, 3, FAKE, N, other, N), _forward(a, 3, FAKE, N, other, N),
                      _solve(a, 3, FAKE, N, other, N)):
        assert code == STATE and "aniso_solve_mixed_dev" in msg, (code, msg)
    with pytest.raises(aniso_amd.AnisoError) as e:
        a.cache_f32()
    assert e.value.code == STATE and "aniso_solve_mixed_dev" in str(e.value)
    assert a.cache_f32_bytes() == 0
    # the argument errors still come first
    assert _mapping(a, 0, 3, None, N, other, N)[0] == INVALID
    assert _solve(a, 3, FAKE, N, other, N, inner_tol=1.0)[0] == INVALID


def test_a_sharded_high_order_handle_is_refused():
    # the handle of the test above is garbage in a reference cycle (pytest.raises holds its
    # frame) and is destroyed when the collector next runs; aniso_destroy, like every call, resets
    # this thread's last error: collect now, so that it cannot fall between a.cache_f32() below and
    # the aniso_last_error that reads its message (as test_sharded_solve_cpu.py does)
    gc.collect()
    a = _handle(np_=6, shard=(0, 2))
    N = a.N
    other = ctypes.c_void_p(4096 + 64 * N * 8)
    for code, msg in (_mapping(a, 0, 3, FAKE, N, other, N), _forward(a, 3, FAKE, N, other, N),
                      _solve(a, 3, FAKE, N, other, N)):
        assert code == STATE and "aniso_create_sharded" in msg, (code, msg)
    with pytest.raises(aniso_amd.AnisoError) as e:
        a.cache_f32()
    assert e.value.code == STATE and "aniso_create_sharded" in str(e.value)


def test_before_mode_0_is_ready_is_a_state_error_that_names_aniso_cache():
    for np_ in (6, 8):
        a = _handle(np_=np_)
        N = a.N
        other = ctypes.c_void_p(4096 + 64 * N * 8)
        for code, msg in (_mapping(a, 0, 3, FAKE, N, other, N), _forward(a, 3, FAKE, N, other, N),
                          _solve(a, 3, FAKE, N, other, N)):
            assert code == STATE and "aniso_cache" in msg, (np_, code, msg)
        with pytest.raises(aniso_amd.AnisoError) as e:
            a.cache_f32()
        assert e.value.code == STATE and "aniso_cache" in str(e.value)
        assert a.cache_f32_bytes() == 0 and a.mode_apply_calls().size == 0
