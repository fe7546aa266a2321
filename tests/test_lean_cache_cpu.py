"""Lean block handles, the part that needs no device: the two new
entries are exported and public, the MEX shim has `cacheBlock`, and aniso_cache_block
checks its arguments and the call order before it touches the GPU."""
import os
import re

import pytest

import aniso_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "integration", "AnisoWrapperMI355X.c")


def test_cache_block_and_cache_bytes_are_exported_and_public():
    public = aniso_amd.exported_symbols(public_only=True)
    lib = aniso_amd.lib()
    for name in ("aniso_cache_block", "aniso_cache_bytes"):
        assert name in aniso_amd.exported_symbols(), name
        assert name in public, name
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    assert callable(aniso_amd.Aniso.cache_block) and callable(aniso_amd.Aniso.cache_bytes)


def test_mex_shim_has_cache_block():
    src = open(SHIM).read()
    ops = set(re.findall(r'!strcmp\(op, "(\w+)"\)', src))
    assert "cacheBlock" in ops
    assert "aniso_cache_block(" in src
    called = set(re.findall(r"\b(aniso_\w+)\(", src))
    exported = set(aniso_amd.exported_symbols())
    assert called <= exported, called - exported
    lib = aniso_amd.lib()
    for name in called:
        assert hasattr(lib, name), name


def test_cache_block_refuses_a_one_block_handle_without_a_device():
    """ks = 1: no block operator on the mode-shared caches -> ANISO_ERR_INVALID, with
    the reason, even before setCoeff (the argument check comes first)."""
    a = aniso_amd.Aniso(8, 1, 1, 0.5, 6, 4, 20)
    with pytest.raises(aniso_amd.AnisoError) as e:
        a.cache_block()
    assert e.value.code == 1
    assert "ks = 1" in str(e.value) and "aniso_cache" in str(e.value)


def test_cache_block_before_set_coeff_is_a_state_error_without_a_device():
    a = aniso_amd.Aniso(8, 1, 5, 0.8, 6, 4, 20)
    with pytest.raises(aniso_amd.AnisoError) as e:
        a.cache_block()
    assert e.value.code == 3
    assert "setCoeff" in str(e.value)


def test_cache_bytes_of_a_fresh_handle_is_zero_without_a_device():
    a = aniso_amd.Aniso(8, 1, 5, 0.8, 6, 4, 20)
    assert a.cache_bytes() == (0, 0)
