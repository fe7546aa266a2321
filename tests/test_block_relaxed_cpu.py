"""The relaxed-precision block solve of a high-order handle, the part that
needs no device: the three entries are exported and declared in the public header with
argtypes and wrappers, aniso_block_solve_relaxed_calls is exported as a development entry, a
fresh handle has recorded no pass, and every refusal comes with its code and a message before
the device is touched."""
import ctypes

import numpy as np
import pytest

import aniso_amd

INVALID, STATE = 1, 3

PUBLIC = {"aniso_block_op_f32_dev": "block_op_f32_dev", "aniso_block_solve_relaxed_dev": "block_solve_relaxed_dev",
          "aniso_block_solve_relaxed": "block_solve_relaxed"}


def _handle(np_=6, ks=2, shard=None):
    return aniso_amd.Aniso(8, 1, ks, 0.5, 6, np_, 20, shard=shard)


def _status(code):
    buf = ctypes.create_string_buffer(4096)
    aniso_amd.lib().aniso_last_error(buf, len(buf))
    return code, buf.value.decode(errors="replace")


def _entries(a, restart=60, tol=1e-11, maxit=20, relax=1e-5):
    """The three public entries on host arrays of the right size (never read: every call here
    is refused before the device is touched), as (name, (code, message))."""
    n = a.ks * a.N
    x, y = np.zeros(n), np.zeros(n)
    px, py = ctypes.c_void_p(x.ctypes.data), ctypes.c_void_p(y.ctypes.data)
    dp = ctypes.POINTER(ctypes.c_double)
    it, rr = ctypes.c_int(), ctypes.c_double()
    L = aniso_amd.lib()
    yield "aniso_block_op_f32_dev", _status(L.aniso_block_op_f32_dev(a.address, 2, px, a.N, py, a.N, 0, None))
    yield "aniso_block_solve_relaxed_dev", _status(L.aniso_block_solve_relaxed_dev(
        a.address, px, py, restart, tol, maxit, relax, None, 0, ctypes.byref(it), ctypes.byref(rr), None))
    yield "aniso_block_solve_relaxed", _status(L.aniso_block_solve_relaxed(
        a.address, x.ctypes.data_as(dp), y.ctypes.data_as(dp), restart, tol, maxit, relax, None, 0, ctypes.byref(it),
        ctypes.byref(rr)))
    assert not x.any() and not y.any()


def _nothing_kept(a):
    assert a.cache_f32_bytes() == 0
    assert a.block_solve_relaxed_calls().size == 0


def test_the_entries_are_public_with_argtypes_and_wrappers():
    public = aniso_amd.exported_symbols(public_only=True)
    for name, wrapper in PUBLIC.items():
        assert name in public, name
        assert getattr(aniso_amd.lib(), name).argtypes is not None, name
        assert callable(getattr(aniso_amd.Aniso, wrapper)), wrapper
    assert "aniso_block_solve_relaxed_calls" in aniso_amd.exported_symbols()
    assert "aniso_block_solve_relaxed_calls" not in public
    assert aniso_amd.lib().aniso_block_solve_relaxed_calls.argtypes is not None
    assert callable(aniso_amd.Aniso.block_solve_relaxed_calls)


def test_a_fresh_handle_has_recorded_no_pass():
    for np_ in (4, 6, 8):
        a = _handle(np_=np_)
        calls = a.block_solve_relaxed_calls()
        assert calls.size == 0 and calls.dtype == np.int32
        code, msg = _status(aniso_amd.lib().aniso_block_solve_relaxed_calls(a.address, None, 0, None))
        assert code == INVALID and msg, (np_, code, msg)


def test_order_4_is_refused_and_pointed_to_the_mixed_solve():
    a = _handle(np_=4)
    for name, (code, msg) in _entries(a):
        assert code == STATE and "aniso_solve_mixed_dev" in msg, (name, code, msg)
    with pytest.raises(aniso_amd.AnisoError) as e:
        a.block_solve_relaxed(np.zeros(a.ks * a.N), restart=60, tol=1e-11, maxit=20)
    assert e.value.code == STATE and "aniso_solve_mixed_dev" in str(e.value)
    _nothing_kept(a)


def test_a_sharded_handle_is_refused():
    for np_ in (6, 8):
        a = _handle(np_=np_, shard=(0, 2))
        for name, (code, msg) in _entries(a):
            assert code == STATE and "aniso_create_sharded" in msg, (np_, name, code, msg)
        _nothing_kept(a)


def test_more_than_8_blocks_are_refused():
    a = _handle(np_=6, ks=9)
    for name, (code, msg) in _entries(a):
        assert code == STATE and "no f32 form" in msg, (name, code, msg)
    _nothing_kept(a)


def test_before_the_caches_is_a_state_error_that_names_both_calls():
    for np_ in (6, 8):
        a = _handle(np_=np_)
        for name, (code, msg) in _entries(a):
            assert code == STATE and "aniso_set_coeff" in msg and "aniso_cache_block" in msg and name in msg, (
                np_, name, code, msg)
        for relax in (0.0, -1.0, 1.0):  # whatever the rule, the same refusal
            for name, (code, msg) in list(_entries(a, relax=relax))[1:]:
                assert code == STATE and "aniso_set_coeff" in msg, (np_, relax, name, code, msg)
        _nothing_kept(a)


@pytest.mark.parametrize("bad", [dict(restart=0), dict(tol=0.0), dict(relax=float("nan")), dict(maxit=0)])
def test_bad_solve_arguments_are_invalid(bad):
    """restart 0, tol 0, maxit 0 and a NaN relax: ANISO_ERR_INVALID from both solve entries (the
    arguments are checked before the handle's state, so a handle without caches shows it)."""
    for np_ in (6, 8):
        a = _handle(np_=np_)
        for name, (code, msg) in list(_entries(a, **bad))[1:]:
            assert code == INVALID and msg, (np_, bad, name, code, msg)
        _nothing_kept(a)


def test_null_pointers_and_a_bad_which_are_invalid():
    a = _handle(np_=6)
    L = aniso_amd.lib()
    x = np.zeros(a.ks * a.N)
    px = ctypes.c_void_p(x.ctypes.data)
    for args in ((2, None, a.N, px, a.N), (2, px, a.N, None, a.N), (3, px, a.N, px, a.N), (-1, px, a.N, px, a.N)):
        code, msg = _status(L.aniso_block_op_f32_dev(a.address, *args, 0, None))
        assert code == INVALID and msg, (args[0], code, msg)
    it, rr = ctypes.c_int(), ctypes.c_double()
    code, msg = _status(L.aniso_block_solve_relaxed_dev(a.address, None, px, 60, 1e-11, 20, 1e-5, None, 0,
                                                        ctypes.byref(it), ctypes.byref(rr), None))
    assert code == INVALID and msg, (code, msg)
