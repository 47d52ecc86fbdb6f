"""The problems of test_gpu_grouped_score.py where there is no GPU: every problem is built, the
claims its GPU test makes about it (work-item and trip counts, scan tiles, merge kernel, group
sizes, dup positions: grouped_problems.assert_*_claims, the same calls the GPU tests make) hold
from the inputs alone, and a handful of its queries go through the oracle: the related list is
the index order the claims were made in, the values are finite, and none of the sample has a
near-tie among its 65 largest (the GPU tests assert that on every query, and then 0 swaps)."""
import numpy as np
import pytest

import grouped_problems as gp
from grouped_problems import SIZES, size_id


def sample_through_oracle(tag, model, k, U, I, train, qu, qi, sample, seed):
    p = gp.params_for(model, U, I, k, seed)
    sample = sorted(set(int(q) for q in sample))
    want = gp.oracle_results(("cpu", tag, model, k), model, k, p, train, qu[sample], qi[sample])
    L = gp.Lists(train, U, I)
    deg_u, deg_i = gp.degrees(train, U, I)
    for q, o in zip(sample, want):
        u, i = int(qu[q]), int(qi[q])
        assert o["n"] == deg_u[u] + deg_i[i]
        assert np.array_equal(o["rel"], np.concatenate([L.rows(0, u), L.rows(1, i)])), (tag, q)
        assert np.isfinite(o["influence"]).all()
    gp.assert_no_near_ties(want)
    return want


@pytest.mark.parametrize("size", SIZES, ids=size_id)
@pytest.mark.parametrize("side", [1, 0], ids=["item-lists", "user-lists"])
def test_edge_problem(size, side):
    model, k = size
    U, I, train, qu, qi, dups, empty, twice = gp.assert_edge_claims(side)
    sample = [dups[0][0], dups[-1][0], twice, empty, empty + 1, qu.size - 1]
    want = sample_through_oracle("edge%d" % side, model, k, U, I, train, qu, qi, sample, 3)
    assert min(o["n"] for o in want) == 0
    Q, total = qu.size, gp.total_related(train, U, I, qu, qi)
    kernels = set(gp.merge_kernel(Q, total, K) for K in gp.KS[model] if K)
    assert kernels >= {"thread", "wave"}, kernels


@pytest.mark.parametrize("size", SIZES, ids=size_id)
def test_group_problem(size):
    model, k = size
    U, I, train, qu, qi, order2 = gp.assert_group_claims()
    # the blocks of every group size, per size of the model's query block
    qb = gp.QB[size]
    blocks = sorted(set((g + qb - 1) // qb for g in gp.GROUPS))
    assert blocks == ([1, 2, 3, 5] if qb == 8 else [1, 2, 3])
    assert set(min(g, qb) if g % qb == 0 else g % qb for g in gp.GROUPS) >= {1, 2, 3, 4, 5, 7, 8}
    sample_through_oracle("groups", model, k, U, I, train, qu, qi, range(0, qu.size, 23), 4)


@pytest.mark.parametrize("size", SIZES, ids=size_id)
def test_trip_problem(size):
    model, k = size
    U, I, train, qu, qi, halves = gp.assert_trip_claims(model, k)
    assert sum(h.size for h in halves) == qu.size
    pairs = np.nonzero(gp.Lists(train, U, I).in_train(qu, qi))[0]
    sample_through_oracle("trips", model, k, U, I, train, qu, qi, [0, qu.size - 1, pairs[0], pairs[-1]], 5)


@pytest.mark.parametrize("nE", gp.TILE_NE)
def test_tile_problem(nE):
    U, I, train, qu, qi = gp.assert_tile_claims(nE)
    for model, k in SIZES:
        sample_through_oracle("tile%d" % nE, model, k, U, I, train, qu, qi, [7, 19, 33], 6)


@pytest.mark.parametrize("size", SIZES, ids=size_id)
@pytest.mark.parametrize("merge", ["wave", "thread"])
def test_long_problem(size, merge):
    model, k = size
    U, I, train, qu, qi, lengths = gp.assert_long_claims(model, k, merge)
    want = sample_through_oracle("long-" + merge, model, k, U, I, train, qu, qi, range(3 * len(lengths)), 7)
    assert [o["n"] >= n for o, n in zip(want[::3], lengths)] == [True] * len(lengths)


def test_subset_problem():
    U, I, train, qu, qi, out_u, out_i = gp.assert_subset_claims()
    sample_through_oracle("subset", "NCF", 32, U, I, train, qu, qi, [0, 12, 16], 9)
