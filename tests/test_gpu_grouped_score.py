"""Oracle tests of the entity-shared VALU scorers (k_score_grouped_mf: MF k in {32, 64} with
top-K >= 2; k_score_ncf: NCF k = 32, any K), of the group builder that feeds only them
(k_group_count, k_group_scan, k_group_fill, k_item_fill) and of the solves and Gram kernels
behind them, at the shapes their index arithmetic depends on -- the lane row of 64, the NCF
one-row path (chunks of <= 64 ratings), the Gram slab of 16, the 256-rating chunk and NCF Gram
slice, the query block of 8 (16 at MF k = 64) and its static column counts 1/2/4/8/16, the
per-query output, slot and position bases in chunks beyond the first, the dup branch (the test
pair's own train row) in every lane row and in chunk 1, the second trip of both grid-stride
loops (k_score_ncf's two-stage header prefetch), the 512-entity tile and 64-tile window of the
group scan, the persistent ranges of k_solve_tile and k_solve, the 4,096-row Gram slices of MF
k = 64, k_record_x and a first prepare that is fia_prepare_for.

Every comparison is against the fp64 oracle (oracle.fia_oracle.CsrExact) unless it says
bitwise: related sets bit-exact, influence and x < RTOL (normalised as rel_err does), top-K
by check_topk with 0 near-tie swaps (no problem has a near-tie among a query's 65 largest:
asserted on the oracle's values).  Which path an input takes is established from the input
alone (grouped_problems.py, whose claims test_grouped_problems_cpu.py also runs).  All problems:
wd = 1e-3, damping = 1e-6, parameters from synth.mf_params / synth.ncf_params."""
import numpy as np
import pytest

import grouped_problems as gp
from grouped_problems import KS, SIZES, oracle_results, params_for, size_id
from test_gpu_mfma_score import RawModel, bits, check_against_oracle
from test_gpu_parity import NEAR_TIE, RTOL, check_topk, make_model, rel_err
from test_gpu_run_score import batch_x

pytestmark = pytest.mark.gpu

assert gp.NEAR_TIE == NEAR_TIE and (gp.WD, gp.DAMPING) == (1e-3, 1e-6)


def checked(res, want, K, tag):
    """check_against_oracle, and no near-tie swap (there is no near-tie to forgive)."""
    worst_i, worst_x, swaps = check_against_oracle(res, want, K, tag)
    assert swaps == 0, (tag, swaps)
    return worst_i, worst_x


def every_K(m, model, k, U, I, train, qu, qi, want, tag):
    """The batch at every K of the model; returns {K: result} and the merge kernels taken
    (from the batch's own Q and total)."""
    out, merges = {}, set()
    for K in KS[model]:
        out[K] = res = m.batch(qu, qi, K)
        checked(res, want, K, "%s %s k=%d K=%d" % (tag, model, k, K))
        if K:
            merges.add(gp.merge_kernel(qu.size, int(res["offsets"][-1]), K))
    assert int(out[KS[model][0]]["offsets"][-1]) == gp.total_related(train, U, I, qu, qi)
    return out, merges


def assert_same_bits(a, b, tag):
    """Two results of the same queries: equal related lists and top-K positions, bit-identical
    influence, x and topk_val."""
    for name in a:
        assert np.array_equal(a[name], b[name], equal_nan=True), (tag, name)
    for name in ("influence", "x", "topk_val"):
        if name in a:
            assert np.array_equal(bits(a[name]), bits(b[name])), (tag, name)


# ---------------------------------------------------------------------------------------
# 1. list-length edges, both sides
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES, ids=size_id)
@pytest.mark.parametrize("side", [1, 0], ids=["item-lists", "user-lists"])
def test_list_length_edges(size, side):
    """Lists of every length at and beside the lane row (64), the NCF one-row path (<= 64), the
    Gram slab (16), the chunk and NCF Gram slice (256) and of 2, 3 and 4 chunks (511..513,
    769), on the item side and, transposed, on the user side; the dup branch at the lists' first
    and last positions and, on the 257- and 513-lists, at 63, 64, 127, 128, 191, 192, 255 and 256
    (every lane row, chunk 1; positions asserted from the index order); a pair that is in train
    twice (positions 5 and 256 of the 257-list); a query with n_q = 0 in the middle of the
    batch.  Every query at every K against CsrExact; the K <= 4 batches take the thread (row)
    merge, the others the wave merge."""
    model, k = size
    U, I, train, qu, qi, dups, empty, twice = gp.assert_edge_claims(side)
    p = params_for(model, U, I, k, 3)
    want = oracle_results(("edge", model, k, side), model, k, p, train, qu, qi)
    gp.assert_no_near_ties(want)
    L = gp.Lists(train, U, I)
    for q, n, pos in dups:                          # the claims' index order is the related lists'
        u, i = int(qu[q]), int(qi[q])
        assert np.array_equal(want[q]["rel"], np.concatenate([L.rows(0, u), L.rows(1, i)])), q
    assert want[empty]["n"] == 0
    m = RawModel(model, k, U, I, train, p)
    out, merges = every_K(m, model, k, U, I, train, qu, qi, want, "edges side=%d" % side)
    assert merges >= {"thread", "wave"}, merges
    for K, res in out.items():
        assert res["offsets"][empty] == res["offsets"][empty + 1]
        # the pair held twice: two train rows, each in both lists, the copies with identical bits
        b, e = res["offsets"][twice], res["offsets"][twice + 1]
        rel, infl = res["rel_idx"][b:e], res["influence"][b:e]
        both = np.unique(rel[np.bincount(rel)[rel] > 1])
        assert both.size == 2
        for row in both:
            assert (rel == row).sum() == 2 and (bits(infl[rel == row]) == bits(infl[rel == row])[0]).all(), (K, row)
    m.close()


# ---------------------------------------------------------------------------------------
# 2. query-group sizes
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES, ids=size_id)
def test_query_group_sizes(size, tmp_path):
    """Item groups of 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17 and 33 queries (asserted) on two-chunk
    lists and on lists of <= 64 ratings: every static column count with and without padding
    columns, groups of several blocks, about half of the queries raters of their item (one
    column of a block on the dup branch, in chunk 0 or 1); a user in 20 queries; a repeated
    query; shuffled batch order.  Every query at every K against CsrExact -- a padding column
    that leaked would overwrite the last query's outputs or slots.  The same queries in a second
    order: per query the same related list and top-K and bit-identical influence, x and
    topk_val (the ranks inside a group come from atomics and from the batch order; the results
    must depend on neither)."""
    model, k = size
    U, I, train, qu, qi, order2 = gp.assert_group_claims()
    p = params_for(model, U, I, k, 4)
    want = oracle_results(("groups", model, k), model, k, p, train, qu, qi)
    gp.assert_no_near_ties(want)
    m = make_model(model, U, I, k, train, (qu, qi), p, tmpdir=tmp_path)
    Q = qu.size
    total = gp.total_related(train, U, I, qu, qi)
    merges = set()
    for K in KS[model]:
        res = m.get_influence_batch(list(range(Q)), K=K)
        assert res["offsets"][-1] == total
        _, _, swaps = check_against_oracle(res, want, K, "groups %s k=%d K=%d" % (model, k, K))
        assert swaps == 0
        merges.add(gp.merge_kernel(Q, total, K))
        shuf = m.get_influence_batch([int(t) for t in order2], K=K)
        offs, soffs = res["offsets"], shuf["offsets"]
        for s, q in enumerate(order2):
            b, e, sb, se = offs[q], offs[q + 1], soffs[s], soffs[s + 1]
            assert np.array_equal(shuf["rel_idx"][sb:se], res["rel_idx"][b:e]), (K, q)
            assert np.array_equal(bits(shuf["influence"][sb:se]), bits(res["influence"][b:e])), (K, q)
            assert np.array_equal(bits(shuf["x"][s]), bits(res["x"][q])), (K, q)
            if K:
                assert np.array_equal(shuf["topk_pos"][s], res["topk_pos"][q]), (K, q)
                assert np.array_equal(bits(shuf["topk_val"][s]), bits(res["topk_val"][q])), (K, q)
    assert merges >= {"thread", "wave"}, merges
    m.ctx.close()


# ---------------------------------------------------------------------------------------
# 3. the second trip of the grid-stride loops
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,K", [(size, K) for size in SIZES for K in KS[size[0]]],
                         ids=lambda v: size_id(v) if isinstance(v, tuple) else "K%d" % v)
def test_second_trip(size, K):
    """Q queries on pairwise distinct users and items of three or four ratings: 2 Q work items
    of one chunk and one block each.  NCF k = 32, Q = 2,060: 4,120 work items on 1,024
    workgroups of 4 waves, so 24 waves take a second trip on headers prefetched during the
    first (words(wi + stride), bounds of the next item; words(wi + 2 stride) clamps to the last
    item), and k_solve_tile runs past its 2,048 resident queries.  MF, Q = 16,400: 32,800 work
    items on 8,192 workgroups, and 32,801 scan words = 65 tiles (a second look-back window).
    300 queries are train pairs, more than k_solve's 256 workgroups.  All of it asserted from
    the input.  Every query against CsrExact; and the two halves of the batch, each a single
    trip, answered on their own equal the big batch bitwise."""
    model, k = size
    U, I, train, qu, qi, halves = gp.assert_trip_claims(model, k)
    p = params_for(model, U, I, k, 5)
    want = oracle_results(("trips", model, k), model, k, p, train, qu, qi)
    gp.assert_no_near_ties(want)
    m = RawModel(model, k, U, I, train, p)
    big = m.batch(qu, qi, K)
    assert int(big["offsets"][-1]) == gp.total_related(train, U, I, qu, qi)
    checked(big, want, K, "second trip %s k=%d K=%d" % (model, k, K))
    offs = big["offsets"]
    for part in halves:
        sub = m.batch(qu[part], qi[part], K)
        q0, q1 = int(part[0]), int(part[-1]) + 1
        cut = dict(offsets=offs[q0:q1 + 1] - offs[q0], rel_idx=big["rel_idx"][offs[q0]:offs[q1]],
                   influence=big["influence"][offs[q0]:offs[q1]], x=big["x"][q0:q1])
        if K:
            cut.update({name: big[name][q0:q1] for name in ("topk_pos", "topk_idx", "topk_val")})
        assert sorted(cut) == sorted(sub)
        assert_same_bits(cut, sub, (model, k, K, q0))
    m.close()


# ---------------------------------------------------------------------------------------
# 4. group-scan tile edges
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES, ids=size_id)
@pytest.mark.parametrize("nE", gp.TILE_NE)
def test_group_scan_tile_edges(size, nE):
    """U + I = 511, 512, 513: the scan's total (index U + I) is the last word of the one tile,
    a tile of its own, the second word of the second tile.  40 queries, the last user and the
    last item among them (together and apart), every one against CsrExact."""
    model, k = size
    U, I, train, qu, qi = gp.assert_tile_claims(nE)
    p = params_for(model, U, I, k, 6)
    want = oracle_results(("tile", nE, model, k), model, k, p, train, qu, qi)
    gp.assert_no_near_ties(want)
    m = RawModel(model, k, U, I, train, p)
    every_K(m, model, k, U, I, train, qu, qi, want, "scan tile U+I=%d" % nE)
    m.close()


# ---------------------------------------------------------------------------------------
# 5. long lists and Gram slices
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES, ids=size_id)
@pytest.mark.parametrize("merge", ["wave", "thread"])
def test_long_lists(size, merge):
    """An item of 2,100 raters: 9 chunks, output base obj + cidx * 256, slot base cbj + cidx and
    position base poj per query of the block.  MF k = 64 also items of 4,095, 4,096, 4,097 and
    8,193 raters: one, one, two and three 4,096-row slices of k_gram_mf_mfma.  Per list a rater
    (its row in a chunk beyond the first: asserted), a non-rater and the user without ratings.
    wave: these queries alone, max_chunks > 16 Q, k_topk_merge at every K; thread: with
    short-list queries, max_chunks <= 16 Q, k_topk_merge_thread (_row at K = 1) for K <= 4
    (asserted from Q and the total)."""
    model, k = size
    U, I, train, qu, qi, lengths = gp.assert_long_claims(model, k, merge)
    p = params_for(model, U, I, k, 7)
    want = oracle_results(("long", merge, model, k), model, k, p, train, qu, qi)
    gp.assert_no_near_ties(want)
    assert all(o["n"] >= n for o, n in zip(want[:3 * len(lengths):3], lengths))
    m = RawModel(model, k, U, I, train, p)
    out, merges = every_K(m, model, k, U, I, train, qu, qi, want, "long lists %s-merge" % merge)
    assert merges == ({"wave"} if merge == "wave" else {"thread", "wave"} | ({"row"} if 1 in KS[model] else set()))
    m.close()


# ---------------------------------------------------------------------------------------
# 6. a given inverse HVP
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES, ids=size_id)
def test_given_inverse_hvp_on_edges(size):
    """fia_query_batch_x on the list-length problem (item lists), K = 2.  Fed the oracle's own
    x: influence and top-K against the oracle -- scoring and k_record_x (dup id, x . v, r-hat)
    without the solve.  Fed fia_query_batch's own x_out: the same related lists as the solve's
    run and influence within 1e-12 relative per query (k_record_x sums x . theta and x . v in
    another order than the solve kernels; the bound of
    test_cached_inverse_hvp_force_refresh_false and test_query_batch_x_on_edges); a doubled x
    gives exactly doubled influence (bitwise)."""
    model, k = size
    K = 2
    U, I, train, qu, qi, dups, empty, twice = gp.assert_edge_claims(1)
    p = params_for(model, U, I, k, 3)
    want = oracle_results(("edge", model, k, 1), model, k, p, train, qu, qi)
    gp.assert_no_near_ties(want)
    m = RawModel(model, k, U, I, train, p)
    D = m.ctx.num_params()
    xo = np.stack([o["x"] if o["n"] else np.zeros(D) for o in want])
    given = batch_x(m, qu, qi, xo, K)
    given["x"] = np.where(np.array([o["n"] for o in want])[:, None] > 0, xo, np.nan)
    checked(given, want, K, "oracle's x %s k=%d" % (model, k))
    first = m.batch(qu, qi, K)
    worst_i, worst_x = checked(first, want, K, "solve run %s k=%d" % (model, k))
    again = batch_x(m, qu, qi, first["x"], K)
    twice_x = batch_x(m, qu, qi, 2.0 * first["x"], K)
    assert np.array_equal(again["offsets"], first["offsets"])
    assert np.array_equal(again["rel_idx"], first["rel_idx"]) and np.array_equal(twice_x["rel_idx"], first["rel_idx"])
    assert np.array_equal(bits(twice_x["influence"]), bits(2.0 * again["influence"]))
    offs = first["offsets"]
    worst = 0.0
    for q, o in enumerate(want):
        b, e = offs[q], offs[q + 1]
        if e == b:
            assert (again["topk_pos"][q] == -1).all()
            continue
        a, f = again["influence"][b:e], first["influence"][b:e]
        err = np.abs(a - f).max() / np.abs(f).max()
        assert err <= 1e-12, (q, err)
        worst = max(worst, err)
        assert rel_err(a, o["influence"]) < RTOL
        assert check_topk(again["topk_pos"][q], a, o["influence"], K) == 0, q
    print("given x %s k=%d: %d queries vs the solve's run, worst influence %.2e (solve run vs oracle: "
          "influence %.2e, x %.2e)" % (model, k, len(want), worst, worst_i, worst_x))
    m.close()


# ---------------------------------------------------------------------------------------
# 7. the first prepare is fia_prepare_for
# ---------------------------------------------------------------------------------------
def test_prepare_for_first_then_ncf_scoring():
    """NCF k = 32: a context whose FIRST prepare is fia_prepare_for -- k_ncf_gram_rows has
    written the list-ordered g_mlp rows and residuals (lgm, lres) that k_score_ncf reads for the
    marked entities only.  The subset (a group of 12 queries on one item: two blocks; a train
    pair; five more) matches the oracle at every K; a query outside the subset is refused in
    between; after a full fia_prepare the same subset is bitwise the same."""
    from influence._lib import FIAError
    model, k = "NCF", 32
    U, I, train, qu, qi, out_u, out_i = gp.assert_subset_claims()
    p = params_for(model, U, I, k, 9)
    want = oracle_results(("subset", model, k), model, k, p, train, qu, qi)
    gp.assert_no_near_ties(want)
    m = RawModel(model, k, U, I, train, p, prepare=False)
    m.prepare_for(qu, qi)
    part, _ = every_K(m, model, k, U, I, train, qu, qi, want, "prepare_for")
    for u, i in ((out_u, int(qi[0])), (int(qu[0]), out_i)):
        with pytest.raises(FIAError):
            m.batch(np.array([u], np.int32), np.array([i], np.int32), 2)
    m.ctx.prepare()
    for K in KS[model]:
        assert_same_bits(part[K], m.batch(qu, qi, K), ("prepare_for", K))
    m.close()
