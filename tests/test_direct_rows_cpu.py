"""Direct evaluation at chosen targets (DESIGN.md "Accuracy of the method"), the part
that needs no device: the four entries are exported, public and documented, and every
refusal is raised before the GPU is touched, with a message naming the argument.  (The
refusal of a mode that is not cached needs aniso_set_coeff, which uploads to the device:
it is checked in test_gpu_direct_rows.py.)"""
import ctypes
import os
import re

import numpy as np
import pytest

import aniso_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("aniso_mapping_direct_dev", "aniso_mapping_direct", "aniso_block_op_direct_dev", "aniso_block_op_direct")
OK, INVALID, STATE, RANGE = 0, 1, 3, 4


def _last_error():
    buf = ctypes.create_string_buffer(4096)
    aniso_amd.lib().aniso_last_error(buf, len(buf))
    return buf.value.decode()


def _i64(v):
    a = np.ascontiguousarray(v, dtype=np.int64)
    return a, a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))


def _handle(ks=3):
    return aniso_amd.Aniso(6, 1, ks, 0.8, 6, 4, 20)  # N = 36; host state only


def _calls(a, targets, nt, ldo=None, which=2, id_=0, null=None):
    """The four entries on handle a with host / fake device pointers (never dereferenced:
    every call here returns before the device is touched).  Yields (name, status)."""
    L = aniso_amd.lib()
    N, ks = a.N, a.ks
    buf = np.zeros(ks * max(N, 1))
    out = np.zeros(ks * max(abs(nt), 1) + 8)
    keep, tp = _i64(targets)
    dp = ctypes.POINTER(ctypes.c_double)
    pin, pout = buf.ctypes.data_as(dp), out.ctypes.data_as(dp)
    vin, vout = ctypes.c_void_p(buf.ctypes.data), ctypes.c_void_p(out.ctypes.data)
    if null == "in":
        pin, vin = None, None
    if null == "out":
        pout, vout = None, None
    if null == "targets":
        tp = None
    ldo = nt if ldo is None else ldo
    yield "aniso_mapping_direct", L.aniso_mapping_direct(a.address, pin, id_, tp, nt, pout)
    yield "aniso_mapping_direct_dev", L.aniso_mapping_direct_dev(a.address, vin, id_, tp, nt, vout, None)
    yield "aniso_block_op_direct", L.aniso_block_op_direct(a.address, which, pin, tp, nt, pout)
    yield "aniso_block_op_direct_dev", L.aniso_block_op_direct_dev(a.address, which, vin, N, tp, nt, vout, ldo, None)
    del keep


def test_entries_are_exported_public_and_documented():
    public = aniso_amd.exported_symbols(public_only=True)
    lib = aniso_amd.lib()
    nargs = {"aniso_mapping_direct_dev": 7, "aniso_mapping_direct": 6, "aniso_block_op_direct_dev": 9,
             "aniso_block_op_direct": 6}
    for n in NAMES:
        assert n in aniso_amd.exported_symbols() and n in public, n
        assert hasattr(lib, n) and len(getattr(lib, n).argtypes) == nargs[n], n
    for w in ("mapping_direct", "mapping_direct_dev", "block_op_direct", "block_op_direct_dev", "fmm_error",
              "block_fmm_error"):
        assert callable(getattr(aniso_amd.Aniso, w)), w
    with open(os.path.join(ROOT, "include", "aniso_mi355x.h")) as f:
        text = f.read()
    at = text.index("int aniso_mapping_direct_dev(")
    doc = re.sub(r"\s*\*?\s+", " ", text[text.rfind("/*", 0, at):at])
    for phrase in ("maxLevel = 0", "nt x N line integrals", "2 sz squares", "does not depend on the number of modes",
                   "ANISO_ERR_INVALID", "ANISO_ERR_RANGE", "ANISO_ERR_STATE", "sharded handle", "nt = 0",
                   "repeats allowed", "ldo >= nt"):
        assert phrase in doc, phrase
    for n in NAMES:
        assert re.search(r"^int %s\(aniso_handle h, " % n, text, re.M), n


def test_nt_zero_is_a_successful_no_op_without_a_device():
    """nt = 0 returns ANISO_OK at once: before aniso_set_coeff, with null pointers."""
    a = _handle()
    for null in (None, "in", "out", "targets"):
        for name, code in _calls(a, [], 0, null=null):
            assert code == OK, (name, null, _last_error())
    assert a.mapping_direct(np.zeros(a.N), 0, []).shape == (0,)
    assert a.block_op_direct(2, np.zeros((a.ks, a.N)), []).shape == (a.ks, 0)


def test_negative_nt_is_invalid():
    a = _handle()
    for name, code in _calls(a, [0], -1):
        assert code == INVALID, name
        assert "nt" in _last_error() and "-1" in _last_error(), (name, _last_error())


@pytest.mark.parametrize("bad", [-1, 36, 2 ** 40])
def test_a_target_outside_the_points_is_invalid(bad):
    a = _handle()
    for name, code in _calls(a, [0, 35, bad, 1], 4):
        msg = _last_error()
        assert code == INVALID, (name, msg)
        assert "targets[2]" in msg and str(bad) in msg and "36" in msg, (name, msg)


def test_null_pointers_with_targets_are_invalid():
    a = _handle()
    word = {"in": ("charge", "x", "u"), "out": ("out",), "targets": ("targets",)}
    for null, words in word.items():
        for name, code in _calls(a, [0, 1], 2, null=null):
            msg = _last_error()
            assert code == INVALID, (name, null, msg)
            assert "NULL" in msg and any(re.search(r"\b%s is NULL" % w, msg) for w in words), (name, null, msg)


def test_ldo_below_nt_is_invalid():
    a = _handle()
    L = aniso_amd.lib()
    keep, tp = _i64([0, 1, 2])
    x = np.zeros(a.ks * a.N)
    out = np.zeros(a.ks * 3)
    code = L.aniso_block_op_direct_dev(a.address, 2, ctypes.c_void_p(x.ctypes.data), a.N, tp, 3,
                                       ctypes.c_void_p(out.ctypes.data), 2, None)
    assert code == INVALID
    assert "ldo" in _last_error() and "nt = 3" in _last_error(), _last_error()
    code = L.aniso_block_op_direct_dev(a.address, 2, ctypes.c_void_p(x.ctypes.data), a.N - 1, tp, 3,
                                       ctypes.c_void_p(out.ctypes.data), 3, None)
    assert code == INVALID and "ldx" in _last_error(), _last_error()


def test_bad_id_and_which():
    a = _handle(ks=3)  # kernel ids 0 .. 4
    got = dict(_calls(a, [0], 1, id_=5))
    assert got["aniso_mapping_direct"] == RANGE and got["aniso_mapping_direct_dev"] == RANGE
    got = dict(_calls(a, [0], 1, id_=-1))
    assert got["aniso_mapping_direct"] == RANGE
    assert "kernel id" in _last_error() or "which" in _last_error() or "setCoeff" in _last_error()
    got = dict(_calls(a, [0], 1, which=3))
    assert got["aniso_block_op_direct"] == INVALID and got["aniso_block_op_direct_dev"] == INVALID


def test_before_set_coeff_is_a_state_error():
    a = _handle()
    for name, code in _calls(a, [0, 5], 2):
        msg = _last_error()
        assert code == STATE, (name, msg)
        assert "setCoeff" in msg and name.replace("_dev", "") in msg, (name, msg)
    with pytest.raises(aniso_amd.AnisoError) as e:
        a.mapping_direct(np.zeros(a.N), 0, [1])
    assert e.value.code == STATE


def test_a_sharded_handle_is_a_state_error():
    """A direct sum needs every source: refused on a shard, whatever else is wrong."""
    a = _handle()
    a.set_shard(0, 2)
    for name, code in _calls(a, [0], 1):
        msg = _last_error()
        assert code == STATE, (name, msg)
        assert "sharded" in msg and "every source" in msg, (name, msg)
    a.set_shard(0, 1)  # one rank: not sharded, the next refusal is the call order
    for name, code in _calls(a, [0], 1):
        assert code == STATE and "setCoeff" in _last_error(), (name, _last_error())


def test_python_rejects_non_integer_targets():
    a = _handle()
    with pytest.raises(aniso_amd.AnisoError) as e:
        a.mapping_direct(np.zeros(a.N), 0, [0.5])
    assert e.value.code == INVALID
