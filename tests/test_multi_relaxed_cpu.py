"""The relaxed-precision multi-source operator and lockstep solves of a high-order handle
(DESIGN.md §3.18.10), the part that needs no device: the five public entries and the
development entry are exported and declared where they belong, with argtypes and wrappers; a
fresh handle has recorded no call; every refusal comes with its code and a message before the
device is touched; counts of 0 are ANISO_OK; the MEX shim compiles with its new op."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import aniso_amd

OK, INVALID, STATE = 0, 1, 3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PUBLIC = {
    "aniso_block_op_multi_f32_dev": "block_op_multi_f32_dev",
    "aniso_block_solve_multi_relaxed_dev": "block_solve_multi_relaxed_dev",
    "aniso_block_solve_multi_relaxed": "block_solve_multi_relaxed",
    "aniso_forward_solve_multi_relaxed_dev": "forward_solve_multi_relaxed_dev",
    "aniso_forward_solve_multi_relaxed": "forward_solve_multi_relaxed",
}
BLOCK = ("aniso_block_op_multi_f32_dev", "aniso_block_solve_multi_relaxed_dev", "aniso_block_solve_multi_relaxed")
# the parameter lists of the issue, as the headers must declare them
SIGNATURES = {
    "aniso_block_op_multi_f32_dev": "h, which, nsrc, x, ldx, out, ldo, stream",
    "aniso_block_solve_multi_relaxed_dev":
        "h, nsrc, q, ldq, rhs_is_charge, x, ldx, restart, tol, maxit, relax, iters, relres, hist, maxhist, stream",
    "aniso_block_solve_multi_relaxed": "h, Q, nsrc, rhs_is_charge, X, restart, tol, maxit, relax, iters, relres",
    "aniso_forward_solve_multi_relaxed_dev":
        "h, nrhs, q, ldq, rhs_is_source, x, ldx, restart, tol, maxit, relax, iters, relres, hist, maxhist, stream",
    "aniso_forward_solve_multi_relaxed": "h, Q, k, rhs_is_source, X, restart, tol, maxit, relax, iters, relres",
    "aniso_solve_multi_relaxed_calls": "h, calls, cap, n",
}


def _handle(np_=6, ks=2, shard=None):
    return aniso_amd.Aniso(8, 1, ks, 0.5, 6, np_, 20, shard=shard)


def _status(code):
    buf = ctypes.create_string_buffer(4096)
    aniso_amd.lib().aniso_last_error(buf, len(buf))
    return code, buf.value.decode(errors="replace")


def _entries(a, n=2, restart=60, tol=1e-11, maxit=20, relax=1e-5, q="q", x="x", ld=None, iters="it"):
    """The five public entries on host arrays of the right size (never read: every call here is
    refused, or has nothing to do, before the device is touched), as (name, (code, message)).
    q / x / iters = None pass NULL; ld is the row stride of the device forms (default N)."""
    rows = max(n, 1) * a.ks
    Q, X = np.zeros((rows, a.N)), np.zeros((rows, a.N))
    it, rr = np.zeros(max(n, 1), dtype=np.int32), np.zeros(max(n, 1))
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
    vq = ctypes.c_void_p(Q.ctypes.data) if q else None
    vx = ctypes.c_void_p(X.ctypes.data) if x == "x" else (vq if x == "q" else None)
    hq = Q.ctypes.data_as(dp) if q else None
    hx = X.ctypes.data_as(dp) if x == "x" else (hq if x == "q" else None)
    pit = it.ctypes.data_as(ip) if iters else None
    prr = rr.ctypes.data_as(dp)
    ld = a.N if ld is None else ld
    L = aniso_amd.lib()
    yield "aniso_block_op_multi_f32_dev", _status(L.aniso_block_op_multi_f32_dev(a.address, 2, n, vq, ld, vx, ld, None))
    yield "aniso_block_solve_multi_relaxed_dev", _status(L.aniso_block_solve_multi_relaxed_dev(
        a.address, n, vq, ld, 1, vx, ld, restart, tol, maxit, relax, pit, prr, None, 0, None))
    yield "aniso_block_solve_multi_relaxed", _status(L.aniso_block_solve_multi_relaxed(
        a.address, hq, n, 1, hx, restart, tol, maxit, relax, pit, prr))
    yield "aniso_forward_solve_multi_relaxed_dev", _status(L.aniso_forward_solve_multi_relaxed_dev(
        a.address, n, vq, ld, 1, vx, ld, restart, tol, maxit, relax, pit, prr, None, 0, None))
    yield "aniso_forward_solve_multi_relaxed", _status(L.aniso_forward_solve_multi_relaxed(
        a.address, hq, n, 1, hx, restart, tol, maxit, relax, pit, prr))
    assert not Q.any() and not X.any()


def _solves(entries):
    return [(name, st) for name, st in entries if "solve" in name]


def _nothing_kept(a):
    assert a.cache_f32_bytes() == 0
    assert a.solve_multi_relaxed_calls().size == 0


def _declaration(header, name):
    text = open(os.path.join(ROOT, "include", header)).read()
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    return None if m is None else ", ".join(p.split()[-1].lstrip("*") for p in m.group(1).split(","))


def test_the_entries_are_exported_and_declared_with_the_issue_s_signatures():
    public = aniso_amd.exported_symbols(public_only=True)
    exported = aniso_amd.exported_symbols()
    for name, wrapper in PUBLIC.items():
        assert name in public and name in exported, name
        assert _declaration("aniso_mi355x.h", name) == SIGNATURES[name], (name, _declaration("aniso_mi355x.h", name))
        assert _declaration("aniso_mi355x_dev.h", name) is None, name
        assert getattr(aniso_amd.lib(), name).argtypes is not None, name
        assert callable(getattr(aniso_amd.Aniso, wrapper)), wrapper
    dev = "aniso_solve_multi_relaxed_calls"
    assert dev in exported and dev not in public
    assert _declaration("aniso_mi355x_dev.h", dev) == SIGNATURES[dev]
    assert _declaration("aniso_mi355x.h", dev) is None
    assert aniso_amd.lib().aniso_solve_multi_relaxed_calls.argtypes is not None
    assert callable(aniso_amd.Aniso.solve_multi_relaxed_calls)


def test_a_fresh_handle_has_recorded_no_call():
    for np_ in (4, 6, 8):
        a = _handle(np_=np_)
        calls = a.solve_multi_relaxed_calls()
        assert calls.shape == (0, 2) and calls.dtype == np.int32
        code, msg = _status(aniso_amd.lib().aniso_solve_multi_relaxed_calls(a.address, None, 0, None))
        assert code == INVALID and msg, (np_, code, msg)


def test_order_4_is_refused_and_pointed_to_the_mixed_solve():
    a = _handle(np_=4)
    for n in (2, 0):  # what the handle rules out comes before the count is looked at
        for name, (code, msg) in _entries(a, n=n):
            assert code == STATE and "aniso_solve_mixed_dev" in msg, (n, name, code, msg)
    with pytest.raises(aniso_amd.AnisoError) as e:
        a.block_solve_multi_relaxed(np.zeros((a.ks * a.N, 2)), restart=60, tol=1e-11, maxit=20)
    assert e.value.code == STATE and "aniso_solve_mixed_dev" in str(e.value)
    with pytest.raises(aniso_amd.AnisoError) as e:
        a.forward_solve_multi_relaxed(np.zeros((a.N, 2)))
    assert e.value.code == STATE and "aniso_solve_mixed_dev" in str(e.value)
    _nothing_kept(a)


def test_more_than_8_blocks_are_refused_by_the_block_entries():
    """ks = 9: the block operator runs as passes, which have no f32 form.  (The forward solve
    uses mode 0 alone, whatever ks: there the next refusal is the missing cache.)"""
    a = _handle(np_=6, ks=9)
    for name, (code, msg) in _entries(a):
        assert code == STATE and msg, (name, code, msg)
        if name in BLOCK:
            assert "no f32 form" in msg, (name, msg)
    _nothing_kept(a)


def test_sharded_handles_are_refused():
    for np_ in (6, 8):
        a = _handle(np_=np_, shard=(0, 2))  # aniso_create_sharded
        for name, (code, msg) in _entries(a):
            assert code == STATE and "aniso_create_sharded" in msg, (np_, name, code, msg)
        _nothing_kept(a)
        a = _handle(np_=np_)
        try:
            a.set_shard(1, 2)  # aniso_set_shard (a high-order handle may refuse the call itself)
        except aniso_amd.AnisoError:
            continue
        for name, (code, msg) in _entries(a):
            assert code == STATE and msg, (np_, name, code, msg)
        _nothing_kept(a)


def test_before_the_coefficients_or_the_caches_is_a_state_error_that_names_the_entry():
    for np_ in (6, 8):
        a = _handle(np_=np_)
        for relax in (1e-5, 0.0, -1.0, 1.0):  # whatever the rule, the same refusal
            for name, (code, msg) in _entries(a, relax=relax):
                assert code == STATE and "aniso_set_coeff" in msg and name in msg, (np_, relax, name, code, msg)
                assert "aniso_cache" in msg, (np_, relax, name, msg)
        _nothing_kept(a)


@pytest.mark.parametrize("bad", [dict(restart=0), dict(restart=401), dict(tol=0.0), dict(tol=-1e-9), dict(maxit=-1),
                                 dict(relax=float("nan"))],
                         ids=["restart0", "restart401", "tol0", "tol<0", "maxit<0", "relaxNaN"])
def test_bad_solve_arguments_are_invalid(bad):
    """The arguments are checked before the handle's state: a handle without caches shows it."""
    for np_ in (6, 8):
        a = _handle(np_=np_)
        for name, (code, msg) in _solves(_entries(a, **bad)):
            assert code == INVALID and msg, (np_, bad, name, code, msg)
        _nothing_kept(a)


@pytest.mark.parametrize("bad", [dict(q=None), dict(x=None), dict(iters=None), dict(ld=-1), dict(x="q")],
                         ids=["q NULL", "x NULL", "iters NULL", "stride N-1", "overlap"])
def test_bad_rows_are_invalid(bad):
    a = _handle(np_=6)
    if bad.get("ld") == -1:
        bad = dict(ld=a.N - 1)
    for name, (code, msg) in _entries(a, **bad):
        if "ld" in bad and not name.endswith("_dev"):
            continue  # the host forms take no stride
        if "iters" in bad and "solve" not in name:
            continue  # the operator has no iters
        assert code == INVALID and msg, (bad, name, code, msg)
    L = aniso_amd.lib()
    x = np.zeros(2 * a.ks * a.N)
    px = ctypes.c_void_p(x.ctypes.data)
    for which in (3, -1):
        code, msg = _status(L.aniso_block_op_multi_f32_dev(a.address, which, 1, px, a.N, px, a.N, None))
        assert code == INVALID and msg, (which, code, msg)
    for name, (code, msg) in _entries(a, n=-1):
        assert code == INVALID and msg, (name, code, msg)
    _nothing_kept(a)


def test_a_count_of_0_is_ok_and_touches_nothing():
    """nsrc = nrhs = 0 with NULL rows, on handles with and without caches."""
    for np_ in (6, 8):
        a = _handle(np_=np_)
        for name, (code, msg) in _entries(a, n=0, q=None, x=None, iters=None):
            assert code == OK, (np_, name, code, msg)
        _nothing_kept(a)


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_the_mex_shim_compiles_with_the_new_op():
    shim = os.path.join(ROOT, "integration", "AnisoWrapperMI355X.c")
    src = open(shim).read()
    assert '"solveMultiRelaxed"' in src and "aniso_block_solve_multi_relaxed(" in src
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-fsyntax-only",
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tests", "mex_stub"), shim])
    assert "solveMultiRelaxed" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
