"""Sharded high-order handles (np = 6, 8), host side, no GPU:
aniso_create_sharded checks its rank / nranks; at np = 4 it is aniso_create followed by
aniso_set_shard; at np = 6, 8 the ranks' own ranges tile [0, N) on leaf boundaries and
every M2L target of the unsharded plan that meets a rank's range is a target there; the
cut rule leaves ranks without points on the smallest shape; a handle made by
aniso_create keeps refusing set_shard."""
import gc

import numpy as np
import pytest

import aniso_amd

G, NS = 0.8, 10
# sz, d, ks, np: the shapes of tests/test_gpu_high_order_shard.py
SHAPES = {"A": (32, 1, 5, 6), "B": (32, 1, 3, 8), "C": (19, 3, 2, 6), "T": (16, 1, 2, 8)}
PLAN_KEYS = ("near_entries", "m2l_entries", "m2l_pairs", "leaves", "m2l_targets", "tree_nodes", "max_leaf", "N",
             "stored_near", "stored_m2l", "m2l_canon", "near_partial", "att_m2l_blocks", "plan_halo_slots",
             "plan_max_lds_slots", "plan_block_reads", "near_loc_entries", "near_corr_rows")


def _make(shape, shard=None):
    sz, d, ks, np_ = SHAPES[shape]
    return aniso_amd.Aniso(sz, d, ks, G, NS, np_, 20, shard=shard)


def test_the_constructor_is_exported():
    assert "aniso_create_sharded" in aniso_amd.exported_symbols(public_only=True)
    assert hasattr(aniso_amd.lib(), "aniso_create_sharded")


@pytest.mark.parametrize("np_", [4, 6, 8])
@pytest.mark.parametrize("rank,nranks", [(0, 0), (0, -1), (-1, 2), (2, 2), (5, 3)])
def test_bad_rank_or_nranks_is_invalid(np_, rank, nranks):
    # (an earlier test's handle that is garbage in a reference cycle is destroyed when the collector
    # next runs, and aniso_destroy, like every call, resets the thread's last error: collect now)
    gc.collect()
    with pytest.raises(aniso_amd.AnisoError) as e:
        aniso_amd.Aniso(16, 1, 2, G, NS, np_, 20, shard=(rank, nranks))
    assert e.value.code == 1 and "nranks" in str(e.value), str(e.value)  # ANISO_ERR_INVALID


@pytest.mark.parametrize("rank,world", [(0, 1), (0, 2), (1, 2), (2, 3), (5, 8)])
def test_np4_is_create_then_set_shard(rank, world):
    a = aniso_amd.Aniso(64, 1, 5, G, NS, 4, 20, shard=(rank, world))
    b = aniso_amd.Aniso(64, 1, 5, G, NS, 4, 20)
    b.set_shard(rank, world)
    assert a.shard() == b.shard()
    assert np.array_equal(a.shard_cuts(world), b.shard_cuts(world))
    assert np.array_equal(a.tree_perm(), b.tree_perm())
    sa, sb = a.stats(), b.stats()
    assert {k: sa[k] for k in PLAN_KEYS} == {k: sb[k] for k in PLAN_KEYS}
    assert a.shard_exchange() == b.shard_exchange() and a.shard_exchange_one() == b.shard_exchange_one()
    assert np.array_equal(a.shard_halo(), b.shard_halo())


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("world", [2, 3, 4, 8])
def test_the_ranks_ranges_cover_the_points_and_the_targets(shape, world):
    full = _make(shape)
    N = full.N
    cuts = full.shard_cuts(world)
    ints, _ = full.tree_nodes()
    parent, is_leaf, is_empty, count, begin = ints[:, 0], ints[:, 7], ints[:, 8], ints[:, 9], ints[:, 10]
    leaves = np.flatnonzero((is_leaf == 1) & (is_empty == 0))
    targets = np.flatnonzero((is_empty == 0) & (parent >= 0))  # the unsharded plan's M2L targets
    assert full.stats()["m2l_targets"] == len(targets) and full.stats()["leaves"] == len(leaves)
    at = 0
    for r in range(world):
        h = _make(shape, shard=(r, world))
        b, e = h.shard()
        assert (b, e) == (int(cuts[r]), int(cuts[r + 1])) and b == at and e >= b, (r, b, e)
        at = e
        # no boundary splits a leaf
        inside = (begin[leaves] >= b) & (begin[leaves] + count[leaves] <= e)
        outside = (begin[leaves] + count[leaves] <= b) | (begin[leaves] >= e)
        assert np.all(inside | outside), r
        assert h.stats()["leaves"] == int(inside.sum()), r
        # every target that intersects the range is a target on this rank (and no other node is)
        meets = (begin[targets] < e) & (begin[targets] + count[targets] > b)
        assert h.stats()["m2l_targets"] == int(meets.sum()), (r, h.stats()["m2l_targets"], int(meets.sum()))
        assert np.array_equal(h.tree_perm(), full.tree_perm())
    assert at == N


def test_shape_t_leaves_the_even_ranks_of_eight_empty():
    """Four 64-point leaves at level 1: the cut rule gives rank r a leaf only where the
    leaf's midpoint passes r N / 8, so the even ranks own nothing."""
    full = _make("T")
    assert full.N == 256 and full.tree_size() == (5, 1)
    assert full.shard_cuts(8).tolist() == [0, 0, 64, 64, 128, 128, 192, 192, 256]
    for r in range(8):
        h = _make("T", shard=(r, 8))
        assert h.n_owned() == (64 if r % 2 else 0), r
        assert h.stats()["leaves"] == r % 2


@pytest.mark.parametrize("np_", [6, 8])
def test_set_shard_stays_refused_on_high_order_handles(np_):
    gc.collect()  # (as above: no aniso_destroy between a refused call and its message)
    a = aniso_amd.Aniso(16, 1, 2, G, NS, np_, 20)
    with pytest.raises(aniso_amd.AnisoError) as e:
        a.set_shard(0, 2)
    assert e.value.code == 1 and "unsharded" in str(e.value), str(e.value)
    s = aniso_amd.Aniso(16, 1, 2, G, NS, np_, 20, shard=(1, 2))  # also on one made by the new constructor
    with pytest.raises(aniso_amd.AnisoError) as e:
        s.set_shard(0, 2)
    assert e.value.code == 1 and "unsharded" in str(e.value), str(e.value)
    assert s.shard() == (128, 256)
    with pytest.raises(aniso_amd.AnisoError) as e:
        s.set_deterministic(True)
    assert e.value.code == 1
    for name, call in (("shard_exchange", s.shard_exchange), ("shard_halo", s.shard_halo)):  # no halo plan
        with pytest.raises(aniso_amd.AnisoError) as e:
            call()
        assert e.value.code == 3 and "sharded high-order" in str(e.value), (name, str(e.value))
