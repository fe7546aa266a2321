"""The resident near field of a high-order handle, the part that needs no
device: the three entries are exported and declared in the public header with argtypes and
wrappers, aniso_mode_near_calls is exported as a development entry, a fresh handle holds no
near blocks, and every refusal comes with its code and a message before the device is touched."""
import ctypes

import pytest

import aniso_amd

INVALID, STATE, RANGE = 1, 3, 4

PUBLIC = {"aniso_cache_mode_near": "cache_mode_near", "aniso_cache_mode_near_bytes": "cache_mode_near_bytes",
          "aniso_cache_mode_near_free": "cache_mode_near_free"}


def _handle(np_=6, ks=2, shard=None):
    return aniso_amd.Aniso(8, 1, ks, 0.5, 6, np_, 20, shard=shard)


def _status(code):
    buf = ctypes.create_string_buffer(4096)
    aniso_amd.lib().aniso_last_error(buf, len(buf))
    return code, buf.value.decode(errors="replace")


def _cache_near(h, id_):
    return _status(aniso_amd.lib().aniso_cache_mode_near(h.address, id_))


def _nothing_kept(a):
    assert a.cache_mode_near_bytes() == 0
    assert len(a.mode_near_calls()) == 0


def test_the_entries_are_public_with_argtypes_and_wrappers():
    public = aniso_amd.exported_symbols(public_only=True)
    for name, wrapper in PUBLIC.items():
        assert name in public, name
        assert getattr(aniso_amd.lib(), name).argtypes is not None, name
        assert callable(getattr(aniso_amd.Aniso, wrapper)), wrapper
    assert "aniso_mode_near_calls" in aniso_amd.exported_symbols()
    assert "aniso_mode_near_calls" not in public
    assert aniso_amd.lib().aniso_mode_near_calls.argtypes is not None
    assert callable(aniso_amd.Aniso.mode_near_calls)


def test_a_fresh_handle_holds_no_near_blocks():
    for np_ in (4, 6, 8):
        a = _handle(np_=np_)
        assert a.cache_mode_near_bytes() == 0
        a.cache_mode_near_free()   # nothing to drop
        a.cache_mode_near_free(0)
        a.cache_mode_free()
        _nothing_kept(a)
        assert a.cache_mode_bytes() == 0
        code, msg = _status(aniso_amd.lib().aniso_cache_mode_near_bytes(a.address, None))
        assert code == INVALID and msg, (np_, code, msg)


def test_a_mode_outside_the_handle_is_a_range_error():
    for np_, ks in ((6, 2), (8, 3), (4, 2)):
        a = _handle(np_=np_, ks=ks)
        for id_ in (-1, 2 * ks - 1, 99):
            code, msg = _cache_near(a, id_)
            assert code == RANGE and "out of range" in msg, (np_, id_, code, msg)
        for id_ in (-2, 2 * ks - 1):
            code, msg = _status(aniso_amd.lib().aniso_cache_mode_near_free(a.address, id_))
            assert code == RANGE and "out of range" in msg, (np_, id_, code, msg)
        _nothing_kept(a)


def test_order_4_is_refused_and_pointed_to_aniso_cache():
    a = _handle(np_=4)
    code, msg = _cache_near(a, 0)
    assert code == STATE and "aniso_cache(h, id)" in msg, (code, msg)
    with pytest.raises(aniso_amd.AnisoError) as e:
        a.cache_mode_near(1)
    assert e.value.code == STATE and "aniso_cache(h, id)" in str(e.value)
    _nothing_kept(a)


def test_a_sharded_handle_is_refused():
    for np_ in (6, 8):
        a = _handle(np_=np_, shard=(0, 2))
        code, msg = _cache_near(a, 0)
        assert code == STATE and "aniso_create_sharded" in msg, (np_, code, msg)
        with pytest.raises(aniso_amd.AnisoError) as e:
            a.cache_mode_near(0)
        assert e.value.code == STATE
        _nothing_kept(a)


def test_before_the_mode_is_ready_is_a_state_error_that_names_both_calls():
    for np_ in (6, 8):
        a = _handle(np_=np_)
        for id_ in (0, 2):
            code, msg = _cache_near(a, id_)
            assert code == STATE and "aniso_cache" in msg and "aniso_set_coeff" in msg, (np_, id_, code, msg)
        with pytest.raises(aniso_amd.AnisoError) as e:
            a.cache_mode_near(0)
        assert e.value.code == STATE and "aniso_cache" in str(e.value) and "aniso_set_coeff" in str(e.value)
        _nothing_kept(a)
        assert a.mode_apply_calls().size == 0
