"""What the parity matrix of tests/test_gpu_high_order_block.py relies on, pinned on the host
(no GPU) from tree_nodes / tree_list: per case the size, the depth, the leaf sizes and the
members of the V, W and X lists its row is listed for -- so that a change to the tree
builder or to a shape cannot quietly empty a case -- and, from the oracle alone, that the
np = 4 operator is a different one at the shapes with a far field.

The pairs a high-order M2L reads transposed (attBlk < 0: a V pair stored once by its smaller
id) are not exposed by name; on a handle without the cluster plan (every
high-order handle) stats() gives the directed reads (hm_block_reads = |attSrc|) and the stored
blocks (att_m2l_blocks = |attOwner|), and every read is one or the other, so their difference
is that count.  It is pinned positive at the cases with W and X lists."""
import functools

import numpy as np
import pytest

import aniso_amd
from conftest import rough_coeffs
from oracle.oracle_py import Oracle

G = 0.8

# sz, d, ks, ns, np, maxLevel: the shapes of tests/test_gpu_high_order_block.py
CASES = {
    "a": (13, 2, 4, 8, 6, 20), "b": (13, 2, 7, 8, 6, 20), "c": (13, 2, 8, 8, 6, 20),
    "d": (11, 3, 5, 8, 8, 20), "e": (11, 3, 6, 8, 8, 20),
    "f": (24, 1, 8, 10, 8, 20), "g": (24, 1, 9, 10, 8, 20),
    "h": (5, 5, 2, 8, 6, 20), "i": (7, 5, 2, 8, 8, 20), "j": (9, 4, 2, 8, 6, 20), "k": (6, 6, 2, 8, 8, 20),
    "l": (15, 3, 2, 8, 8, 2), "m": (12, 2, 3, 8, 6, 1), "n": (8, 2, 2, 8, 6, 0), "o": (1, 6, 1, 8, 8, 20),
    "p": (16, 1, 1, 10, 6, 20),
}

# N, nodes, depth, smallest and largest leaf, members of the V, W and X lists
FACTS = {
    "a": (676, 69, 3, 9, 36, 564, 52, 52), "b": (676, 69, 3, 9, 36, 564, 52, 52), "c": (676, 69, 3, 9, 36, 564, 52, 52),
    "d": (1089, 49, 3, 12, 64, 420, 60, 60), "e": (1089, 49, 3, 12, 64, 420, 60, 60),
    "f": (576, 21, 2, 36, 36, 156, 0, 0), "g": (576, 21, 2, 36, 36, 156, 0, 0),
    "h": (625, 53, 3, 6, 36, 282, 54, 54), "i": (1225, 81, 3, 16, 64, 1056, 20, 20),
    "j": (1296, 85, 3, 16, 25, 1272, 0, 0), "k": (1296, 85, 3, 16, 25, 1272, 0, 0),
    "l": (2025, 21, 2, 121, 144, 156, 0, 0), "m": (576, 5, 1, 144, 144, 0, 0, 0),
    "n": (256, 1, 0, 256, 256, 0, 0, 0), "o": (36, 1, 0, 36, 36, 0, 0, 0), "p": (256, 21, 2, 16, 16, 156, 0, 0),
}

# the property each row of the matrix is listed for
WX_LISTS = ("a", "b", "c", "d", "e", "h", "i")
DEPTH_3 = ("a", "b", "c", "d", "e", "h", "i", "j", "k")
OVER_64 = ("l", "m", "n")     # k_ho_p2m and k_ho_l2p loop
OVER_128 = ("l", "m", "n")    # three P2M chunks
NO_V_PAIR = ("m", "n", "o")
ONE_NODE = ("n", "o")


@functools.lru_cache(maxsize=None)
def _tree(case):
    sz, d, ks, ns, np_, ml = CASES[case]
    a = aniso_amd.Aniso(sz, d, ks, G, ns, np_, ml)
    ints, _ = a.tree_nodes()
    leaf = (ints[:, 7] == 1) & (ints[:, 8] == 0)
    lists = [int(a.tree_list(w)[0][-1]) for w in range(4)]  # U, V, W, X
    return dict(N=a.N, nn=ints.shape[0], depth=int(ints[:, 5].max()), leaf_min=int(ints[leaf, 9].min()),
                leaf_max=int(ints[leaf, 9].max()), V=lists[1], W=lists[2], X=lists[3], np=np_, stats=a.stats())


@pytest.mark.parametrize("case", sorted(CASES))
def test_the_tree_of_every_case_is_the_one_the_matrix_names(case):
    t = _tree(case)
    got = (t["N"], t["nn"], t["depth"], t["leaf_min"], t["leaf_max"], t["V"], t["W"], t["X"])
    assert got == FACTS[case], (case, got)
    assert t["N"] <= 2025


def test_every_row_has_the_property_it_is_listed_for():
    for c in WX_LISTS:
        assert _tree(c)["W"] > 0 and _tree(c)["X"] > 0, c
    for c in DEPTH_3:
        assert _tree(c)["depth"] >= 3, c
    for c in OVER_64:
        assert _tree(c)["leaf_max"] > 64, c
    for c in OVER_128:
        assert _tree(c)["leaf_max"] > 128, c
    for c in NO_V_PAIR:
        assert _tree(c)["V"] == 0 and _tree(c)["stats"]["m2l_pairs"] == 0, c
    for c in ONE_NODE:
        assert _tree(c)["nn"] == 1, c
    # the leaves of the np = 8 cases with lists reach the capacity 64 (one lane per point in P2M)
    assert _tree("d")["leaf_max"] == 64 and _tree("i")["leaf_max"] == 64
    # the uniform cases f, g, p and the capped l have a far field: V pairs, M2M and L2L levels
    for c in ("f", "g", "l", "p"):
        assert _tree(c)["V"] == 156 and _tree(c)["depth"] == 2, c


@pytest.mark.parametrize("case", ["a", "d", "h", "i"])
def test_some_v_pairs_are_stored_once_and_read_transposed(case):
    s = _tree(case)["stats"]
    transposed = s["hm_block_reads"] - s["att_m2l_blocks"]
    print(f"case {case}: {s['hm_block_reads']} block reads, {s['att_m2l_blocks']} stored, {transposed} transposed")
    assert s["hm_clusters"] == 0  # no cluster plan: hm_block_reads counts the directed att reads
    assert s["hm_block_reads"] == s["m2l_pairs"]  # every V, W and X pair is one read
    assert 0 < transposed < s["att_m2l_blocks"], (case, s)


@pytest.mark.parametrize("case", ["a", "d", "h"])
def test_order_4_is_a_different_operator_at_these_trees(case):
    """Mode 0 of the np = 4 oracle against the oracle at the case's order on a uniform random
    charge: more than 1e-6 apart (1.5e-3 to 5.8e-3 measured), so a block kernel that ran rank
    16, or dropped the far field, cannot pass the 1e-10 parity bound."""
    sz, d, _, ns, np_, ml = CASES[case]
    q = np.random.default_rng(5).uniform(-1.0, 1.0, sz * sz * d * d)
    out = {}
    for order in (4, np_):
        o = Oracle(sz, d, 1, G, ns, order, ml)
        o.setCoeff(*rough_coeffs(o.getNodes(), 7))
        o.cache(0)
        out[order] = o.mapping(q, 0)
        o.close()
    diff = float(np.linalg.norm(out[4] - out[np_]) / np.linalg.norm(out[np_]))
    print(f"case {case}: np 4 against np {np_} oracle, mode 0: {diff:.3e}")
    assert diff > 1e-6, diff
