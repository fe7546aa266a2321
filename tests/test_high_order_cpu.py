"""High-order handles (np = 6, 8), host side, no GPU: aniso_create
accepts Chebyshev orders 4, 6 and 8 and nothing else; the geometry does not depend on
the order; the quadtree is built with leaf capacity np^2 and is bit-identical to the
oracle's restatement of bbfmm::tree at that rank; a high-order handle is unsharded."""
import numpy as np
import pytest

import aniso_amd
from oracle.oracle_py import OTree


@pytest.mark.parametrize("np_", [6, 8])
def test_create_accepts_order_6_and_8(np_):
    a = aniso_amd.Aniso(16, 3, 2, 0.5, 8, np_, 20)
    assert a.N == 16 * 16 * 9 and a.np == np_
    assert a.num_blocks() == 2


@pytest.mark.parametrize("np_", [3, 5, 7, 10])
def test_create_refuses_other_orders(np_):
    with pytest.raises(aniso_amd.AnisoError) as e:
        aniso_amd.Aniso(16, 3, 1, 0.5, 8, np_, 20)
    assert e.value.code == 1, e.value.code  # ANISO_ERR_INVALID
    assert "4, 6 or 8" in str(e.value), str(e.value)  # the message names the accepted set


@pytest.mark.parametrize("np_", [6, 8])
def test_geometry_does_not_depend_on_the_order(np_):
    a4 = aniso_amd.Aniso(13, 3, 1, 0.5, 10, 4, 20)
    a = aniso_amd.Aniso(13, 3, 1, 0.5, 10, np_, 20)
    assert a.N == a4.N
    assert np.array_equal(a.getNodes(), a4.getNodes())
    assert np.array_equal(a.getWeights(), a4.getWeights())


# a uniform shape, an odd-sz d = 3 shape (non-uniform tree) and a maxLevel-capped shape
@pytest.mark.parametrize("sz,d,ml", [(32, 1, 20), (11, 3, 20), (40, 2, 2)])
@pytest.mark.parametrize("np_", [6, 8])
def test_tree_and_lists_bit_exact_vs_oracle_at_rank_np2(np_, sz, d, ml):
    a = aniso_amd.Aniso(sz, d, 1, 0.5, 8, np_, ml)
    xy = a.getNodes()
    ot = OTree(xy[:, 0], xy[:, 1], np_ * np_, ml)
    ints, geom = a.tree_nodes()
    oi, og = ot.node_ints(), ot.node_geom()
    assert ints.shape[0] == ot.nn
    assert np.array_equal(ints[:, :10], oi[:, :10])
    assert np.array_equal(geom, og)
    for w in range(4):
        ptr, idx = a.tree_list(w)
        ol = ot.lists(w)
        for i in range(ot.nn):
            assert np.array_equal(idx[ptr[i]:ptr[i + 1]], ol[i]), (w, i)
    perm = a.tree_perm()
    assert np.array_equal(np.sort(perm), np.arange(a.N))
    for i in range(ot.nn):
        if ints[i, 7]:  # leaves: same point order as the reference's sourceIndex
            assert np.array_equal(perm[ints[i, 10]:ints[i, 10] + ints[i, 9]], ot.sources(i))
    leaf = ints[:, 7] == 1
    assert ints[leaf, 9].max() <= np_ * np_ or ints[:, 5].max() == ml  # capacity np^2 unless maxLevel cuts it
    if ml == 2:
        assert ints[leaf, 9].max() > np_ * np_  # the capped shape does hold fuller leaves


@pytest.mark.parametrize("np_", [6, 8])
def test_high_order_handles_are_unsharded(np_):
    a = aniso_amd.Aniso(16, 1, 2, 0.5, 8, np_, 20)
    with pytest.raises(aniso_amd.AnisoError) as e:
        a.set_shard(0, 2)
    assert e.value.code == 1 and "unsharded" in str(e.value), str(e.value)
    a.set_shard(0, 1)  # one rank is the whole handle
    assert a.shard() == (0, a.N)
    with pytest.raises(aniso_amd.AnisoError) as e:
        a.set_deterministic(True)
    assert e.value.code == 1 and str(e.value)
    a.set_deterministic(False)
