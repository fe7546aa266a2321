"""One mode on several vectors on a lean np = 4 handle, the part that
needs no device: aniso_mode_apply_calls is exported (a development entry) and reports no
pass on a fresh handle, and the argument and state errors of the multi entries on an np = 4
handle come with their codes before the device is touched (null or fake device pointers)."""
import ctypes

import numpy as np
import pytest

import aniso_amd

INVALID, STATE, RANGE = 1, 3, 4
FAKE = ctypes.c_void_p(4096)  # a non-null "device pointer" no check may follow


def _handle(ks=2):
    return aniso_amd.Aniso(8, 1, ks, 0.5, 6, 4, 20)


def _status(code):
    buf = ctypes.create_string_buffer(4096)
    aniso_amd.lib().aniso_last_error(buf, len(buf))
    return code, buf.value.decode(errors="replace")


def _calls(a, counts, cap, n):
    return _status(aniso_amd.lib().aniso_mode_apply_calls(a.address, counts, cap, n))


def test_mode_apply_calls_is_exported_as_a_development_entry():
    assert "aniso_mode_apply_calls" in aniso_amd.exported_symbols()
    assert "aniso_mode_apply_calls" not in aniso_amd.exported_symbols(public_only=True)
    fn = aniso_amd.lib().aniso_mode_apply_calls
    assert fn.argtypes is not None
    assert callable(aniso_amd.Aniso.mode_apply_calls)


def test_a_fresh_handle_reports_no_pass():
    a = _handle()
    n = ctypes.c_int(-1)
    assert _calls(a, None, 0, ctypes.byref(n))[0] == 0 and n.value == 0
    counts = (ctypes.c_int * 4)(9, 9, 9, 9)
    n = ctypes.c_int(-1)
    assert _calls(a, counts, 4, ctypes.byref(n))[0] == 0 and n.value == 0
    assert list(counts) == [9, 9, 9, 9]
    got = a.mode_apply_calls()
    assert got.shape == (0,) and got.dtype == np.int32
    code, msg = _calls(a, None, 0, None)  # n is required
    assert code == INVALID and msg, (code, msg)


def test_refused_calls_leave_no_pass_behind():
    """Argument errors, an id out of range, a call before set_coeff and a sharded handle: each
    raised on an np = 4 handle with no device present, and none recorded as a pass."""
    lib = aniso_amd.lib()
    a = _handle()
    N = a.N
    other = ctypes.c_void_p(4096 + 64 * N * 8)

    def mapping(h, id_, nrhs, x, ldx, out, ldo):
        return _status(lib.aniso_mapping_multi_dev(h.address, id_, nrhs, x, ldx, out, ldo, None))

    def forward(h, nrhs, x, ldx, out, ldo):
        return _status(lib.aniso_forward_multi_dev(h.address, nrhs, x, ldx, out, ldo, None))

    for args in [(-1, FAKE, N, other, N), (2, FAKE, N - 1, other, N), (2, FAKE, N, other, N - 1),
                 (2, None, N, other, N), (2, FAKE, N, None, N)]:
        assert mapping(a, 0, *args)[0] == INVALID, args
        assert forward(a, *args)[0] == INVALID, args
    for id_ in (-1, 2 * a.ks - 1, 99):
        code, msg = mapping(a, id_, 2, FAKE, N, other, N)
        assert code == RANGE and "out of range" in msg, (id_, code, msg)
    code, msg = forward(a, 2, FAKE, N, ctypes.c_void_p(4096 + 8 * N), N)
    assert code == INVALID and "overlap" in msg, (code, msg)
    for code, msg in (mapping(a, 1, 11, FAKE, N, other, N), forward(a, 11, FAKE, N, other, N)):
        assert code == STATE and "aniso_set_coeff" in msg and "aniso_cache" in msg, (code, msg)
    Q = np.zeros((N, 11), order="F")
    with pytest.raises(aniso_amd.AnisoError) as e:
        a.mapping_multi(Q, 0)
    assert e.value.code == STATE
    assert a.mode_apply_calls().size == 0
    s = _handle()
    s.set_shard(0, 2)
    for code, msg in (mapping(s, 0, 11, FAKE, N, other, N), forward(s, 11, FAKE, N, other, N)):
        assert code == STATE and "sharded" in msg, (code, msg)
    assert s.mode_apply_calls().size == 0
    assert mapping(a, 0, 0, None, N, None, N)[0] == 0  # nothing to do is still nothing to do
    assert a.mode_apply_calls().size == 0
