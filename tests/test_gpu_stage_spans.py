"""aniso_set_timing on the four un-fused routes: the high-order block
apply, the high-order and the lean rank-16 mode apply, and the multi-source block apply.
Each records the same spans at each timing level, and the timers change no bit of the
output (these routes sum in a fixed order).

One shape: sz = 32, d = 1, ks = 3, ns = 10, g = 0.8, maxLevel = 20, demo.m's constant
coefficients (N = 1,024) -- two up tiers at np = 4 and 6, one level of 16 leaves at np = 8.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SZ, D, KS, NS, G, ML = 32, 1, 3, 10, 0.8, 20
# level -> the keys that are positive; every other key (exchange, gather, ...) is exactly 0
POSITIVE = {1: ("near", "corr", "up", "m2l", "down", "total"), 2: ("near", "m2l", "total")}


def _torch():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


@functools.lru_cache(maxsize=None)
def _handle(np_):
    """A handle with every mode ready by aniso_cache_block alone; left as found."""
    import aniso_amd

    a = aniso_amd.Aniso(SZ, D, KS, G, NS, np_, ML)
    xy = a.getNodes()
    a.setCoeff(20.0 + 0.0 * xy[:, 0], 20.2 + 0.0 * xy[:, 0])  # demo.m: sigma_s = 20, sigma_a = 0.2
    a.cache_block()
    if np_ == 4:
        assert a.cache_bytes()[0] == 0  # lean: no per-mode operators
    return a


@functools.lru_cache(maxsize=None)
def _rows(nrows, N):
    torch = _torch()
    return torch.tensor(np.random.default_rng(nrows + N).uniform(-1.0, 1.0, (nrows, N)), device="cuda")


def _check(case):
    torch = _torch()
    route, np_ = case.rsplit("-np", 1)
    a = _handle(int(np_))
    if route == "block":  # aniso_block_op_dev, which = 2
        X = _rows(KS, a.N)
        call = lambda out: a.block_op_dev(2, X, out)  # noqa: E731
    elif route == "multi":  # aniso_block_op_multi_dev, which = 2, 3 sources
        X = _rows(3 * KS, a.N)
        call = lambda out: a.block_op_multi_dev(2, X, out)  # noqa: E731
    else:  # aniso_mapping_multi_dev, mode 1, 3 columns
        X = _rows(3, a.N)
        call = lambda out: a.mapping_multi_dev(X, 1, out)  # noqa: E731
    outs, times = {}, {}
    for level in (0, 1, 2):
        out = torch.zeros_like(X)
        a.set_timing(level)
        for _ in range(2):
            call(out)
        a.sync()
        times[level] = a.stage_times()
        a.set_timing(0)
        outs[level] = out.cpu().numpy()
    if case == "mode-lean16-np4":
        assert list(a.mode_apply_calls()) == [4]  # the mode-kernel route, 3 columns padded to 4
    print(case, {lv: {k: round(v, 5) for k, v in t.items()} for lv, t in times.items()})
    assert np.all(np.isfinite(outs[0])) and np.any(outs[0] != 0.0)
    for level in (1, 2):
        assert np.array_equal(outs[level], outs[0]), level
        assert len(times[level]) == 8 and set(POSITIVE[level]) <= set(times[level])
        for k, t in times[level].items():
            if k in POSITIVE[level]:
                assert t > 0, (level, k, times[level])
            else:
                assert t == 0, (level, k, times[level])


def test_stage_spans_block_np6():
    _check("block-np6")


def test_stage_spans_block_np8():
    _check("block-np8")


def test_stage_spans_mode_np6():
    _check("mode-np6")


def test_stage_spans_mode_lean16_np4():
    _check("mode-lean16-np4")


def test_stage_spans_multi_np6():
    _check("multi-np6")
