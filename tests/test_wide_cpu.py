"""The wide setting of a high-order handle, the part that needs no device:
aniso_set_wide / aniso_get_wide are exported and declared in the public header with the
header's signatures, argtypes and wrappers; a fresh handle has the setting off; every refusal
comes with its code and a message before the device is touched."""
import ctypes
import os
import re

import pytest

import aniso_amd

INVALID, STATE = 1, 3

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "aniso_mi355x.h")


def _handle(np_=6, ks=2, shard=None):
    return aniso_amd.Aniso(8, 1, ks, 0.5, 6, np_, 20, shard=shard)


def _status(code):
    buf = ctypes.create_string_buffer(4096)
    aniso_amd.lib().aniso_last_error(buf, len(buf))
    return code, buf.value.decode(errors="replace")


def _set(h, on):
    return _status(aniso_amd.lib().aniso_set_wide(h.address, on))


def _get(h):
    v = ctypes.c_int(-7)
    code = aniso_amd.lib().aniso_get_wide(h.address, ctypes.byref(v))
    assert code == 0
    return v.value


def test_the_entries_are_public_with_the_headers_signatures():
    public = aniso_amd.exported_symbols(public_only=True)
    text = re.sub(r"\s+", " ", open(HEADER).read())
    assert "int aniso_set_wide(aniso_handle h, int on);" in text
    assert "int aniso_get_wide(aniso_handle h, int *on);" in text
    L = aniso_amd.lib()
    for name in ("aniso_set_wide", "aniso_get_wide"):
        assert name in public, name
    assert L.aniso_set_wide.argtypes == [ctypes.c_void_p, ctypes.c_int]
    assert L.aniso_get_wide.argtypes == [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]
    assert callable(aniso_amd.Aniso.set_wide) and isinstance(aniso_amd.Aniso.wide, property)


def test_off_by_default_and_the_wrapper_round_trips():
    for np_ in (6, 8):
        a = _handle(np_=np_)
        assert _get(a) == 0 and a.wide is False
        a.set_wide()
        assert _get(a) == 1 and a.wide is True
        a.set_wide(True)   # a second call changes nothing
        assert a.wide is True
        a.set_wide(False)
        assert _get(a) == 0 and a.wide is False
        assert _set(a, 1)[0] == 0 and a.wide is True
        # a setting, not a cache: the free calls keep it (new coefficients: the GPU tests)
        a.cache_mode_free()
        a.cache_mode_near_free()
        assert a.wide is True
        assert a.mode_apply_calls().size == 0 and a.cache_mode_bytes() == 0


def test_order_4_refuses_on_and_accepts_off():
    a = _handle(np_=4)
    code, msg = _set(a, 1)
    assert code == STATE and "np = 6, 8" in msg and "aniso_set_wide" in msg, (code, msg)
    assert _get(a) == 0
    with pytest.raises(aniso_amd.AnisoError) as e:
        a.set_wide()
    assert e.value.code == STATE and "np = 6, 8" in str(e.value)
    code, msg = _set(a, 0)
    assert code == 0 and _get(a) == 0, (code, msg)
    a.set_wide(False)


def test_a_sharded_handle_refuses_on_and_accepts_off():
    for np_ in (6, 8):
        a = _handle(np_=np_, shard=(0, 2))
        code, msg = _set(a, 1)
        assert code == STATE and "aniso_create_sharded" in msg and "aniso_set_wide" in msg, (np_, code, msg)
        assert _get(a) == 0
        assert _set(a, 0)[0] == 0
    a = _handle(np_=4, shard=(1, 2))   # an aniso_set_shard rank: order 4's refusal comes first
    code, msg = _set(a, 1)
    assert code == STATE and "np = 6, 8" in msg, (code, msg)
    assert _set(a, 0)[0] == 0 and _get(a) == 0


def test_any_other_value_and_a_null_pointer_are_invalid():
    for np_ in (4, 6):
        a = _handle(np_=np_)
        for on in (2, -1, 16):
            code, msg = _set(a, on)
            assert code == INVALID and "must be 0 or 1" in msg and str(on) in msg, (np_, on, code, msg)
        code, msg = _status(aniso_amd.lib().aniso_get_wide(a.address, None))
        assert code == INVALID and "on is NULL" in msg, (np_, code, msg)
        assert _get(a) == 0
