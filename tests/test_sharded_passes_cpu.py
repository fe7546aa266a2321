"""Host-only pins of the sharded ks > 8 block operator: the plan
flags that decide each case's route in tests/test_gpu_sharded_passes.py (so a planner
change that silently moves a case to another route is noticed), and the contract the
header states."""
import os
import re

import pytest

import aniso_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# sz, d, maxLevel, world, ks -> per rank: one-collective plan ok, upper partials on, records, owned points
PLANS = [
    ((32, 1, 20, 2, 9), [1, 1], [0, 0], [0, 0], [512, 512]),
    ((48, 1, 20, 2, 9), [1, 1], [1, 1], [0, 0], [1152, 1152]),
    ((64, 1, 20, 2, 17), [1, 1], [1, 1], [0, 0], [2048, 2048]),
    ((96, 1, 20, 3, 12), [1, 1, 1], [1, 1, 1], [6, 6, 6], [3024, 3168, 3024]),
    ((64, 1, 20, 3, 12), [0, 0, 1], [0, 0, 1], [0, 0, 0], [1344, 1408, 1344]),
    ((64, 1, 20, 2, 12), [1, 1], [1, 1], [0, 0], [2048, 2048]),
    ((40, 1, 3, 2, 9), [1, 1], [0, 0], [0, 0], [800, 800]),
    ((32, 2, 20, 2, 10), [1, 1], [1, 1], [0, 0], [2048, 2048]),
    ((128, 1, 20, 4, 12), [1, 1, 1, 1], [1, 1, 1, 1], [4, 4, 4, 4], [4096, 4096, 4096, 4096]),
    ((128, 1, 20, 8, 12), [1] * 8, [1] * 8, [2] * 8, [2048] * 8),  # the loopback case: rank 3 of 8
]


@pytest.mark.parametrize("case,oks,ups,recs,owned", PLANS, ids=[f"sz{c[0][0]}d{c[0][1]}ml{c[0][2]}w{c[0][3]}ks{c[0][4]}" for c in PLANS])
def test_plan_flags_of_the_sharded_pass_cases(case, oks, ups, recs, owned):
    sz, d, ml, world, ks = case
    assert aniso_amd.block_pass_plan(ks) == (8, (ks + 7) // 8)
    got = []
    for r in range(world):
        h = aniso_amd.Aniso(sz, d, ks, 0.8, 10, 4, ml)
        h.set_shard(r, world)
        up = h.shard_upper_partials()
        got.append((h.shard_exchange_one()["ok"], up["on"], up["records"], h.n_owned()))
    assert got == list(zip(oks, ups, recs, owned))


def _comment_before(text, decl):
    """The comment block that ends right before the declaration `decl`."""
    at = text.index(decl)
    start = text.rfind("/*", 0, at)
    assert start >= 0
    return re.sub(r"\s*\*?\s+", " ", text[start:at])


def test_header_states_the_sharded_contract():
    with open(os.path.join(ROOT, "include", "aniso_mi355x.h")) as f:
        text = f.read()
    one = _comment_before(text, "int aniso_block_op_sharded_dev(")
    assert "any ks" in one and "ks > 8" in one, one
    two = _comment_before(text, "int aniso_block_op_begin_dev(")
    assert "ks > 8" in two and "ANISO_ERR_INVALID" in two and "aniso_block_op_sharded_dev" in two, two
