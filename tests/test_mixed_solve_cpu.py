"""Host-only pins of the general mixed-precision solve (aniso_solve_mixed_dev, DESIGN.md
§3.14): the symbols and their headers, the refusals that need no device, and the routing
of aniso_amd.solve.gmres_mixed."""
import ctypes
import gc
import os
import re

import numpy as np
import pytest

import aniso_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "aniso_solve_mixed_dev"
DEV = ("aniso_arnoldi16_work_size", "aniso_arnoldi16_begin", "aniso_arnoldi16_step", "aniso_arnoldi16_solution")


def test_symbol_is_exported_public_and_declared():
    assert NAME in aniso_amd.exported_symbols()
    assert NAME in aniso_amd.exported_symbols(public_only=True)
    lib = aniso_amd.lib()
    assert hasattr(lib, NAME)
    assert len(getattr(lib, NAME).argtypes) == 16
    assert callable(aniso_amd.Aniso.solve_mixed_dev)
    with open(os.path.join(ROOT, "include", "aniso_mi355x.h")) as f:
        text = f.read()
    at = text.index(f"int {NAME}(")
    doc = re.sub(r"\s*\*?\s+", " ", text[text.rfind("/*", 0, at):at])
    for phrase in ("main.cpp:121-141", "1 <= m <= 400", "groups of 16", "(m + 1) x 16 x N floats",
                   "ANISO_ERR_RUNTIME", "longest_cycle"):
        assert phrase in doc, phrase


def test_development_entries_are_exported_and_not_public():
    names, public = aniso_amd.exported_symbols(), aniso_amd.exported_symbols(public_only=True)
    lib = aniso_amd.lib()
    for n in DEV:
        assert n in names and n not in public, n
        assert getattr(lib, n).argtypes is not None, n
    for w in ("arnoldi16_work", "arnoldi16_begin", "arnoldi16_step", "arnoldi16_solution"):
        assert callable(getattr(aniso_amd.Aniso, w)), w
    ns, npart = ctypes.c_int64(), ctypes.c_int64()
    assert lib.aniso_arnoldi16_work_size(100, ctypes.byref(ns), ctypes.byref(npart)) == 0
    one = ctypes.c_int64()
    assert lib.aniso_arnoldi_state_size(100, ctypes.byref(one)) == 0
    assert ns.value == 16 * one.value and npart.value >= 16 * 102
    for m in (0, 401):
        assert lib.aniso_arnoldi16_work_size(m, ctypes.byref(ns), ctypes.byref(npart)) == 1, m


def _call(h, nrhs, ld, m, buf):
    o, i, lc = ctypes.c_int(7), ctypes.c_int(7), ctypes.c_int(7)
    code = aniso_amd.lib().aniso_solve_mixed_dev(h.address, nrhs, buf.ctypes.data, ld, buf.ctypes.data, ld, m, 1e-12,
                                                 1e-6, 30, 20, ctypes.byref(o), ctypes.byref(i), ctypes.byref(lc), None,
                                                 None)
    msg = ctypes.create_string_buffer(1024)
    aniso_amd.lib().aniso_last_error(msg, len(msg))
    assert (o.value, i.value, lc.value) == (7, 7, 7)
    return code, msg.value.decode()


def test_refusals_come_before_the_device():
    """ANISO_ERR_INVALID (1) for the arguments, ANISO_ERR_STATE (3) for the handle's
    state: no device exists here, and the dummy host pointers are never read."""
    gc.collect()  # (a collected handle's aniso_destroy would reset the last error between the calls below)
    h = aniso_amd.Aniso(8, 1, 1, 0.8, 10, 4, 20)
    N = h.N
    buf = np.zeros(3 * N)
    for what, (nrhs, ld, m), word in (("m = 0", (3, N, 0), "[1, 400]"), ("m = 401", (3, N, 401), "[1, 400]"),
                                      ("nrhs = 0", (0, N, 80), "nrhs"), ("ldb < N", (3, N - 1, 80), "leading dimension")):
        code, msg = _call(h, nrhs, ld, m, buf)
        assert code == 1 and word in msg, (what, code, msg)
    code, msg = _call(h, 3, N, 80, buf)  # valid arguments: the handle has no coefficients
    assert code == 3 and "before setCoeff" in msg, (code, msg)
    h.set_shard(0, 2)
    code, msg = _call(h, 3, N, 80, buf)
    assert code == 3 and "sharded" in msg, (code, msg)
    assert not buf.any()
    # the 16-row entry keeps its own bound
    code16 = aniso_amd.lib().aniso_solve16_mixed_dev(h.address, buf.ctypes.data, N, buf.ctypes.data, N, 40, 1e-12, 1e-6,
                                                     30, 20, None, None, None, None)
    assert code16 == 3


class _Routed(Exception):
    pass


class _Stub:
    """Records the first solve-level method gmres_mixed reaches; the library solves
    return zeros, the torch loop's first operator call ends the run."""

    N = 32

    def __init__(self, owned=None):
        self.calls = []
        self._owned = self.N if owned is None else owned

    def n_owned(self):
        return self._owned

    def solve16_mixed_dev(self, B, X, **kw):
        self.calls.append(("solve16_mixed_dev", kw["m"]))
        return 2, 11, np.zeros(B.shape[0])

    def solve_mixed_dev(self, B, X, **kw):
        self.calls.append(("solve_mixed_dev", kw["m"]))
        return 2, 11, 9, np.zeros(B.shape[0])

    def forward16_f64_dev(self, X, Y):
        self.calls.append(("torch loop", None))
        raise _Routed

    def apply_block_dev(self, *a, **kw):
        self.calls.append(("torch loop", None))
        raise _Routed

    def tree_perm(self):
        return np.arange(self.N)


def _fake_cuda(torch, t):
    """A CPU tensor that says it is on the device: the routing reads is_cuda, dtype and
    the shape before it hands the tensor to the (stubbed) solve."""

    class OnDevice(torch.Tensor):
        is_cuda = property(lambda self: True)

    return t.as_subclass(OnDevice)


def test_gmres_mixed_routing():
    torch = pytest.importorskip("torch")
    from aniso_amd.solve import gmres_mixed

    def route(rows, m, cuda=True, op=None, **kw):
        op = op or _Stub()
        B = torch.ones(rows, _Stub.N, dtype=torch.float64)
        try:
            out = gmres_mixed(op, _fake_cuda(torch, B) if cuda else B, m=m, **kw)
            assert len(out) == 4 and tuple(out[0].shape) == (rows, _Stub.N)
        except _Routed:
            pass
        assert len(op.calls) == 1, op.calls
        return op.calls[0]

    assert route(16, 40) == ("solve16_mixed_dev", 40)
    assert route(16, 47) == ("solve16_mixed_dev", 47)
    assert route(16, 80) == ("solve_mixed_dev", 80)
    assert route(16, 48) == ("solve_mixed_dev", 48)
    assert route(5, 40) == ("solve_mixed_dev", 40)
    assert route(40, 400) == ("solve_mixed_dev", 400)
    assert route(5, 40, cuda=False) == ("torch loop", None)
    assert route(16, 40, cuda=False) == ("torch loop", None)
    assert route(5, 401) == ("torch loop", None)
    assert route(5, 40, op=_Stub(owned=_Stub.N // 2)) == ("torch loop", None)  # a sharded handle
    assert route(5, 40, native=False) == ("torch loop", None)
