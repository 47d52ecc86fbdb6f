"""Oracle tests of the k <= 16 item-run scoring kernels (k_score_mf_runs: MF k in {8, 16};
k_score_ncf_runs: NCF k in {8, 16}) at the shapes their index arithmetic depends on -- the
chunk (128 ratings per MF descriptor, two per lane: lane rows idx and idx + 64; 64 per NCF
descriptor), the run (k_query_scan<1> cuts runs of equal consecutive test items at item
changes and at every multiple of 16 of the batch index; the head scores the item chunk for
all nq queries, each with its own output base, candidate-slot base, 1/n, c_q and dup id),
the cost-8 slices (an item descriptor costs nq + 2 <= 18), the 512-query scan tile, the dup
branch (the test pair's own train row) at lane row 1, in later chunks and for single queries
of a run, the top-1 fast path (an f32 max that resolves f32-equal keys exactly), both top-K
merge kernels fed from these kernels' candidate slots, and k_record_x's record words.

Every comparison is against the fp64 oracle (oracle.fia_oracle.CsrExact) unless it says
bitwise: related sets bit-exact, influence and x < RTOL (normalised as rel_err does), top-K
by check_topk, topk_idx = rel[pos], topk_val the bits of influence[pos], unused slots
-1 / NaN.  Which path an input takes is established from the input alone (the scan's run
rule, list positions from the index order, the merge-branch rule, the oracle's values).  All
problems: wd = 1e-3, damping = 1e-6, parameters from synth.mf_params / synth.ncf_params."""
import functools

import numpy as np
import pytest

from influence import synth
from test_gpu_mfma_score import RawModel, bits, check_against_oracle
from test_gpu_parity import NEAR_TIE, RTOL, check_topk, make_model, rel_err

pytestmark = pytest.mark.gpu

WD, DAMPING = 1e-3, 1e-6
SIZES = [("MF", 8), ("MF", 16), ("NCF", 8), ("NCF", 16)]
SIZES_MIXED = [("MF", 16), ("NCF", 8), ("MF", 8), ("NCF", 16)]
CLEN = {"MF": 128, "NCF": 64}            # kRunChunk, kNcfRunChunk
RUN_QB = 16                              # kRunQB
SCAN_TILE = 512                          # kScanTile


def size_id(v):
    return "%s-%d" % v if isinstance(v, tuple) else None


def params_for(model, U, I, k, seed):
    return synth.mf_params(U, I, k, seed) if model == "MF" else synth.ncf_params(U, I, k, seed)


_ORACLE_CACHE = {}


def oracle_results(key, model, k, p, train, qu, qi):
    """CsrExact results (rel, n, influence, x) of every query, computed once per problem and
    shared (read-only); a pair that occurs twice in a batch is solved once."""
    from oracle import fia_oracle as fo
    if key not in _ORACLE_CACHE:
        tu, ti, tr = train
        ex = fo.CsrExact(model, p, k, tu, ti, tr, WD, DAMPING)
        memo = {}
        out = []
        for u, i in zip(qu, qi):
            pair = (int(u), int(i))
            if pair not in memo:
                o = ex.query(*pair)
                memo[pair] = {name: o[name] for name in ("rel", "n", "influence", "x")}
            out.append(memo[pair])
        _ORACLE_CACHE[key] = out
    return _ORACLE_CACHE[key]


def scan_runs(qi):
    """The (head, nq) runs k_query_scan<1> cuts a batch into: a query is a run head when its
    batch index is a multiple of 16 or the query before it has another test item."""
    out = []
    q, Q = 0, len(qi)
    while q < Q:
        e = q + 1
        while e < Q and e % RUN_QB and qi[e] == qi[q]:
            e += 1
        out.append((q, e - q))
        q = e
    return out


# ---------------------------------------------------------------------------------------
# 1. list-length edges, both sides
# ---------------------------------------------------------------------------------------
LENGTHS = [1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 385]
DUP_LISTS = (129, 193, 257)              # also queried by the raters at DUP_AT
DUP_AT = (63, 64, 127, 128)              # lane row 0's last entry, lane row 1's first and last, chunk 2's first
EDGE_SEED = 41


@functools.lru_cache(maxsize=None)
def edge_problem(side):
    """One long-list entity per length in LENGTHS plus one without ratings (side 1: items hold
    the lists; side 0: the transposed problem, users hold them), the train rows permuted so
    that list order is train-row order and not id order.  Per list: the raters at the first and
    the last list position (their pairs are train rows: the dup branch at both ends), for the
    129-, 193- and 257-lists also the raters at positions 63, 64, 127 and 128, a non-rater with
    a non-empty list and the entity with no ratings; one pair on the unrated list; the batch
    is item-major, and one query with n_q = 0 sits in its middle.
    Returns U, I, train, qu, qi, dups [(query, list position of its own train row)], the
    index of the empty query."""
    rng = np.random.default_rng(EDGE_SEED)
    U, I = 520, len(LENGTHS) + 1
    raters = [rng.choice(U - 1, n, replace=False).astype(np.int32) for n in LENGTHS]
    tu = np.concatenate(raters)
    ti = np.concatenate([np.full(r.size, j, np.int32) for j, r in enumerate(raters)])
    N = tu.size
    perm = rng.permutation(N)
    tu, ti = tu[perm], ti[perm]
    tr = rng.integers(1, 6, N).astype(np.float32)
    deg_u = np.bincount(tu, minlength=U)
    qs = []                                        # (user, item, list position of the pair's row or -1)
    for j, n in enumerate(LENGTHS):
        order = tu[ti == j]                        # item j's list in index (train-row) order
        at = sorted({0, n - 1} | (set(DUP_AT) if n in DUP_LISTS else set()))
        qs += [(int(order[pos]), j, pos) for pos in at]
        others = np.setdiff1d(np.nonzero(deg_u > 0)[0], order)
        qs += [(int(rng.choice(others)), j, -1), (U - 1, j, -1)]
    qs.append((int(raters[5][0]), I - 1, -1))
    empty = (U - 1, I - 1, -1)
    if side == 0:
        U, I, tu, ti = I, U, ti, tu
        qs = [(i, u, pos) for u, i, pos in qs]
        qs = [qs[t] for t in np.argsort([q[1] for q in qs], kind="stable")]     # item-major
        empty = (U - 1, I - 1, -1)
    mid = len(qs) // 2
    qs.insert(mid, empty)
    qu = np.array([q[0] for q in qs], np.int32)
    qi = np.array([q[1] for q in qs], np.int32)
    dups = [(t, q[2]) for t, q in enumerate(qs) if q[2] >= 0]
    assert N == sum(LENGTHS) and qu.size == 72 and len(dups) == 40
    return U, I, (tu, ti, tr), qu, qi, dups, mid


def assert_dup_positions(train, qu, qi, dups, want, side):
    """The train row of each dup query's pair sits at the stated position of the long side's
    list (the related list gives the index order: user rows, then item rows)."""
    tu, ti, _ = train
    deg_u = np.bincount(tu, minlength=int(qu.max()) + 1)
    seen = set()
    for q, pos in dups:
        row = np.nonzero((tu == qu[q]) & (ti == qi[q]))[0]
        assert row.size == 1, q
        du = deg_u[qu[q]]
        part = want[q]["rel"][du:] if side == 1 else want[q]["rel"][:du]
        assert part[pos] == row[0], (q, pos)
        seen.add((part.size, pos))
    for n in LENGTHS:
        assert (n, 0) in seen and (n, n - 1) in seen, n
    for n in DUP_LISTS:
        for pos in DUP_AT:
            assert (n, pos) in seen, (n, pos)


@pytest.mark.parametrize("size", SIZES, ids=size_id)
@pytest.mark.parametrize("side", [1, 0], ids=["item-lists", "user-lists"])
def test_list_length_edges(size, side, tmp_path):
    """Lists of every length at and beside both chunk sizes and the MF lane-row boundary
    (1, 2, 63..65, 127..129, 191..193, 255..257, 385: three full MF chunks plus one rating, six
    NCF chunks plus one), on the item side and, transposed, on the user side; the dup branch at
    list positions 0, 63, 64, 127, 128 and at the list's end (asserted from the index order);
    a query with n_q = 0 in the middle of the batch; K = 0, 1 and 4 (the three kernel
    variants).  Every query of every batch against CsrExact."""
    model, k = size
    U, I, train, qu, qi, dups, empty = edge_problem(side)
    p = params_for(model, U, I, k, 3)
    want = oracle_results(("edge", model, k, side), model, k, p, train, qu, qi)
    assert_dup_positions(train, qu, qi, dups, want, side)
    assert want[empty]["n"] == 0 and 0 < empty < qu.size - 1
    m = make_model(model, U, I, k, train, (qu, qi), p, tmpdir=tmp_path)
    for K in (0, 1, 4):
        res = m.get_influence_batch(list(range(qu.size)), K=K)
        assert res["offsets"][empty] == res["offsets"][empty + 1]
        check_against_oracle(res, want, K, "run edges %s k=%d side=%d K=%d" % (model, k, side, K))
    m.ctx.close()


# ---------------------------------------------------------------------------------------
# 2. run lengths, run cuts and per-query bases
# ---------------------------------------------------------------------------------------
RUN_U = 400                               # users of the run problem; RUN_U - 1 has no ratings
HEAVY = {0: 63, 1: 64, 2: 65, 3: 128, 4: 130, 5: 131}     # user -> degree (on short-list items only)
ONES = np.arange(380, RUN_U - 1)          # users of degree 1
N_LONG, N_FILL = 10, 140                  # items 0..9: 140..158 ratings; then 140 short-list items
LONG_RATERS = 2100
RUN_GROUPS = [1, 2, 15, 16, 17, 31, 32, 33, 40]
# No order of the nine groups behind the leading group of 5 yields every run length 1..16
# (all 9! orders tried: at best two lengths are missing), so a few queries on short-list items
# (a new item each: the batch stays item-major) shift the groups' start residues mod 16:
# RUN_SPACERS[j] queries go in front of group j.
RUN_SPACERS = [0, 1, 0, 2, 1, 0, 2, 0, 3]


@functools.lru_cache(maxsize=None)
def run_problem(long_item=False):
    """Ten items of 140 to 158 ratings (2 MF chunks, 3 NCF chunks) rated by users of degree
    ~4 and by the degree-1 users; six users of degree 63, 64, 65, 128, 130 and 131 on 140
    short-list items; one user without ratings.  long_item: one more item, rated by 2100
    further users (of degree 1).  Train rows permuted."""
    rng = np.random.default_rng(52)
    U = RUN_U + (LONG_RATERS if long_item else 0)
    I = N_LONG + N_FILL + (1 if long_item else 0)
    pool = np.arange(len(HEAVY), ONES[0])
    us, its = [], []
    for j in range(N_LONG):
        mine = ONES[ONES % N_LONG == j]
        r = np.concatenate([rng.choice(pool, 140 + 2 * j - mine.size, replace=False), mine])
        us.append(r)
        its.append(np.full(r.size, j))
    for h, d in HEAVY.items():
        us.append(np.full(d, h))
        its.append(N_LONG + rng.choice(N_FILL, d, replace=False))
    if long_item:
        us.append(np.arange(RUN_U, U))
        its.append(np.full(LONG_RATERS, I - 1))
    tu = np.concatenate(us).astype(np.int32)
    ti = np.concatenate(its).astype(np.int32)
    perm = rng.permutation(tu.size)
    tu, ti = tu[perm], ti[perm]
    tr = rng.integers(1, 6, tu.size).astype(np.float32)
    deg_u = np.bincount(tu, minlength=U)
    assert all(deg_u[h] == d for h, d in HEAVY.items()) and (deg_u[ONES] == 1).all() and deg_u[RUN_U - 1] == 0
    return U, I, (tu, ti, tr)


@functools.lru_cache(maxsize=None)
def run_batch():
    """The item-major batch of section 2: a group of 5 on item 9, then groups of RUN_GROUPS[j]
    queries on item j (behind RUN_SPACERS[j] queries on a short-list item).  A group's users
    are non-raters of its item, about half of them from the users of degree 0, 1, 63..65 and
    ~130.  In the first 16-run three queries (head, middle, last) are raters of the item, at
    list positions 0, 70 and the last; in the second 16-run one query is repeated.
    Returns qu, qi, the two run heads."""
    U, I, (tu, ti, _) = run_problem()
    rng = np.random.default_rng(53)
    deg_i = np.bincount(ti, minlength=I)
    special = np.concatenate([np.arange(len(HEAVY)), ONES, [RUN_U - 1]])
    short_items = iter(N_LONG + np.nonzero(deg_i[N_LONG:] > 0)[0])
    plan = [(5, N_LONG - 1)]
    for j, (g, s) in enumerate(zip(RUN_GROUPS, RUN_SPACERS)):
        if s:
            plan.append((s, int(next(short_items))))
        plan.append((g, j))
    qu, qi = [], []
    for g, item in plan:
        cand = np.setdiff1d(np.arange(RUN_U), tu[ti == item])
        w = np.where(np.isin(cand, special), 8.0, 1.0)
        qu += [int(u) for u in rng.permutation(rng.choice(cand, g, replace=False, p=w / w.sum()))]
        qi += [item] * g
    qu, qi = np.array(qu, np.int32), np.array(qi, np.int32)
    heads = [h for h, nq in scan_runs(qi) if nq == RUN_QB and qi[h] < N_LONG]
    for t, h in enumerate(heads):                   # every 16-run: user lists of different chunk counts
        qu[h + 3] = (RUN_U - 1, 4, 5)[t % 3]
        qu[h + 11] = (0, 1, 2, 3)[t % 4]
    h_dup, h_rep = heads[0], heads[1]
    lst = tu[ti == qi[h_dup]]                       # the item's list in index order
    qu[h_dup], qu[h_dup + 7], qu[h_dup + 15] = lst[0], lst[70], lst[-1]
    qu[h_rep + 5] = qu[h_rep + 4]
    return qu, qi, h_dup, h_rep


def spread_order(qi):
    """A fixed order of the batch in which equal test items are never adjacent (query t of a
    group of g at key (t + 1/2) / g): every run is a run of one."""
    key = np.empty(qi.size)
    for item in np.unique(qi):
        at = np.nonzero(qi == item)[0]
        key[at] = (np.arange(at.size) + 0.5) / at.size
    return np.argsort(key, kind="stable")


@pytest.mark.parametrize("size", SIZES, ids=size_id)
def test_run_lengths(size, tmp_path):
    """Item groups of 1, 2, 15, 16, 17, 31, 32, 33 and 40 queries on two-MF-chunk (three-NCF-
    chunk) lists, starting at batch indices that are no multiples of 16: the scan's rule cuts
    them into runs of every length 1..16 (asserted from the batch; an item descriptor of a run
    costs nq + 2, 3..18 against slices of 8).  The users of a run have degrees 0, 1, 63..65 and
    ~130: different user-chunk counts, output bases, slot bases and 1/n inside one run.  One
    16-run holds three raters of its item (head, middle, last; list positions 0, 70 and the
    last: the dup branch for one query while its neighbours take the plain path on the same
    chunk), another the same query twice.  K = 0, 1, 4, 64, every query against CsrExact; and
    the same queries in an order without adjacent equal items (runs of one): per query the same
    related list and top-K positions and bit-identical influence, x and topk_val (e_j depends
    on the entity only and s_j on the query only)."""
    model, k = size
    U, I, train = run_problem()
    tu, ti, _ = train
    qu, qi, h_dup, h_rep = run_batch()
    Q = qu.size
    # the preconditions, from the inputs
    groups = [(int(v), int((qi == v).sum())) for v in qi[np.sort(np.unique(qi, return_index=True)[1])]]
    assert [g for v, g in groups if v < N_LONG] == [5] + RUN_GROUPS
    starts = np.nonzero(np.diff(qi, prepend=-1))[0]
    assert len(starts) == len(groups), "item-major"
    assert all(s % RUN_QB for s in starts[1:] if qi[s] < N_LONG)
    runs = scan_runs(qi)
    assert set(nq for h, nq in runs if qi[h] < N_LONG) == set(range(1, RUN_QB + 1))
    deg_u, deg_i = np.bincount(tu, minlength=U), np.bincount(ti, minlength=I)
    assert all(140 <= deg_i[v] <= 160 for v, g in groups if v < N_LONG)
    in_train = np.array([((tu == u) & (ti == i)).any() for u, i in zip(qu, qi)])
    assert sorted(np.nonzero(in_train)[0]) == [h_dup, h_dup + 7, h_dup + 15]
    assert (h_dup, RUN_QB) in runs and (h_rep, RUN_QB) in runs
    assert qu[h_rep + 4] == qu[h_rep + 5] and qi[h_rep + 4] == qi[h_rep + 5]
    for h, nq in runs:
        if nq == RUN_QB and qi[h] < N_LONG:
            d = set(deg_u[qu[h:h + nq]])
            assert len(set((v + CLEN[model] - 1) // CLEN[model] for v in d)) >= 2, h    # user-chunk counts differ
    for want_deg in (0, 1, 63, 64, 65, 128, 130, 131):
        assert (deg_u[qu] == want_deg).any(), want_deg
    order = spread_order(qi)
    assert all(nq == 1 for h, nq in scan_runs(qi[order]))
    p = params_for(model, U, I, k, 4)
    want = oracle_results(("runs", model, k), model, k, p, train, qu, qi)
    lst = np.nonzero(ti == qi[h_dup])[0]
    for q, pos in ((h_dup, 0), (h_dup + 7, 70), (h_dup + 15, lst.size - 1)):
        assert want[q]["rel"][deg_u[qu[q]] + pos] == lst[pos] and tu[lst[pos]] == qu[q]
    m = make_model(model, U, I, k, train, (qu, qi), p, tmpdir=tmp_path)
    for K in (0, 1, 4, 64):
        res = m.get_influence_batch(list(range(Q)), K=K)
        check_against_oracle(res, want, K, "run lengths %s k=%d K=%d" % (model, k, K))
        shuf = m.get_influence_batch([int(t) for t in order], K=K)
        offs, soffs = res["offsets"], shuf["offsets"]
        for s, q in enumerate(order):
            b, e, sb, se = offs[q], offs[q + 1], soffs[s], soffs[s + 1]
            assert np.array_equal(shuf["rel_idx"][sb:se], res["rel_idx"][b:e]), (K, q)
            assert np.array_equal(bits(shuf["influence"][sb:se]), bits(res["influence"][b:e])), (K, q)
            assert np.array_equal(bits(shuf["x"][s]), bits(res["x"][q])), (K, q)
            if K:
                assert np.array_equal(shuf["topk_pos"][s], res["topk_pos"][q]), (K, q)
                assert np.array_equal(bits(shuf["topk_val"][s]), bits(res["topk_val"][q])), (K, q)
    m.ctx.close()


# ---------------------------------------------------------------------------------------
# 3. more than one scan tile; both merge kernels
# ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tile_batch():
    """Q = 1100 item-major queries on the run problem's ten long items (three scan tiles of
    512): groups of 1..40 queries, one group over the batch indices 500..530 and one over
    1010..1040 (runs up to, and from, the tile boundaries 512 and 1024)."""
    rng = np.random.default_rng(54)
    Q = 1100
    qi = np.empty(Q, np.int32)
    item, q = 0, 0
    for lo, hi, whole in ((0, 500, False), (500, 531, True), (531, 1010, False), (1010, 1041, True),
                          (1041, Q, False)):
        while q < hi:
            g = hi - q if whole else min(hi - q, int(rng.integers(1, 41)))
            item = (item + 1 + int(rng.integers(0, N_LONG - 1))) % N_LONG      # another item than the last group's
            qi[q:q + g] = item
            q += g
    qu = rng.integers(0, RUN_U, Q).astype(np.int32)
    return qu, qi


@functools.lru_cache(maxsize=None)
def merge_batch(merge):
    """The 2100-rater item queried by a rater, by a non-rater of degree 128 and by the user
    without ratings (wave merge: Q = 3), plus 12 queries on the two-chunk items (thread merge)."""
    U, I, (tu, ti, _) = run_problem(long_item=True)
    rng = np.random.default_rng(55)
    qs = [(int(tu[ti == I - 1][0]), I - 1), (3, I - 1), (RUN_U - 1, I - 1)]
    if merge == "thread":
        qs += [(int(u), int(i)) for u, i in zip(rng.integers(0, RUN_U, 12), rng.integers(0, N_LONG, 12))]
    return np.array([q[0] for q in qs], np.int32), np.array([q[1] for q in qs], np.int32)


@pytest.mark.parametrize("size", SIZES_MIXED, ids=size_id)
@pytest.mark.parametrize("case", ["tiles", "wave-merge", "thread-merge"])
def test_two_scan_tiles_and_merges(size, case, tmp_path):
    """tiles: 1100 queries (three scan tiles), an item group over the batch indices 500..530 and
    one over 1010..1040, so runs end at and start from the boundaries of the 512-query tile (the
    run lengths there are read from the next tile's items); K = 1, every query against CsrExact.
    merges: an item of 2100 raters (17 MF / 33 NCF chunks: candidate slots slot base + co / chunk).
    The merge kernel is chosen by max_chunks = 2 Q + total_rel / clen + 1 <= 16 Q (K <= 4), clen
    = 128 (MF) / 64 (NCF): Q = 3 -> k_topk_merge (a wave per query), Q = 15 ->
    k_topk_merge_thread (asserted from the batch's own Q and total).  Top-1 position, train row
    and value against the oracle in both."""
    from oracle import fia_oracle as fo
    model, k = size
    if case == "tiles":
        U, I, train = run_problem()
        qu, qi = tile_batch()
        assert qu.size > 2 * SCAN_TILE
        assert (qi[500:531] == qi[500]).all() and qi[499] != qi[500] != qi[531]
        assert (qi[1010:1041] == qi[1010]).all() and qi[1009] != qi[1010] != qi[1041]
        runs = scan_runs(qi)
        for r in ((500, 12), (512, 16), (528, 3), (1010, 14), (1024, 16), (1040, 1)):
            assert r in runs, r
        p = params_for(model, U, I, k, 4)
        m = make_model(model, U, I, k, train, (qu, qi), p, tmpdir=tmp_path)
        res = m.get_influence_batch(list(range(qu.size)), K=1)
        want = oracle_results(("tiles", model, k), model, k, p, train, qu, qi)
        check_against_oracle(res, want, 1, "scan tiles %s k=%d" % (model, k))
        m.ctx.close()
        return
    merge = case.split("-")[0]
    U, I, train = run_problem(long_item=True)
    qu, qi = merge_batch(merge)
    p = params_for(model, U, I, k, 5)
    m = make_model(model, U, I, k, train, (qu, qi), p, tmpdir=tmp_path)
    res = m.get_influence_batch(list(range(qu.size)), K=1)
    Q, total = qu.size, int(res["offsets"][-1])
    max_chunks = 2 * Q + total // CLEN[model] + 1
    assert (max_chunks > 16 * Q) == (merge == "wave"), (Q, total, max_chunks)
    want = oracle_results(("merge", model, k, merge), model, k, p, train, qu, qi)
    assert all(o["n"] >= LONG_RATERS for o in want[:3])
    check_against_oracle(res, want, 1, "long list %s k=%d %s-merge" % (model, k, merge))
    for q in range(3):
        o = want[q]
        a = np.sort(np.abs(o["influence"]))
        got = int(res["topk_pos"][q][0])
        if a[-1] - a[-2] > NEAR_TIE * a[-1]:             # no near-tie at the top: the oracle's position
            assert got == int(fo.topk(o["influence"], 1)[0]), (q, got)
        assert abs(abs(o["influence"][got]) - a[-1]) <= NEAR_TIE * a[-1], (q, got)
        assert res["topk_idx"][q][0] == o["rel"][got]
        assert abs(res["topk_val"][q][0] - o["influence"][got]) < RTOL * a[-1]
    m.ctx.close()


# ---------------------------------------------------------------------------------------
# 4. the top-1 fast path's tie handling
# ---------------------------------------------------------------------------------------
TIE_N = 129                               # raters per item: two MF chunks, three NCF chunks
TIE_OTHERS = (3, 70, 127, 128)            # the twin's list position
# (the twin's position, whether the fp64-larger key sits at the lower position); then the
# bit-identical copies (below / above top)
TIE_SPECS = [(o, low) for o in TIE_OTHERS for low in (True, False)] + [("below", None), ("above", None)]
TIE_SEED = 0                              # of the synth parameters


def top_pair_ok(infl, top, other):
    """The oracle-side preconditions of a tie case: the pair is ranks 1 and 2, equal after
    rounding to float32 and different in fp64; rank 3 is more than 1e-6 (relative) below."""
    from oracle import fia_oracle as fo
    first = fo.topk(infl, 3)
    a, b, c = abs(infl[top]), abs(infl[other]), abs(infl[first[2]])
    return bool(set(first[:2]) == {top, other} and np.float32(a) == np.float32(b) and a != b and
                min(a, b) - c > 1e-6 * max(a, b))


def copy_pair_ok(infl, top, other):
    """... of an exact-copy case: the pair is ranks 1 and 2, equal up to the oracle's own
    rounding; rank 3 is more than 1e-6 (relative) below."""
    from oracle import fia_oracle as fo
    first = fo.topk(infl, 3)
    a, b, c = abs(infl[top]), abs(infl[other]), abs(infl[first[2]])
    return bool(set(first[:2]) == {top, other} and abs(a - b) <= NEAR_TIE * a and min(a, b) - c > 1e-6 * a)


TIE_POOL = 40                             # items to build the cases on (each case takes the first that works)


@functools.lru_cache(maxsize=None)
def tie_problem(model, k):
    """TIE_POOL items of 129 raters each (disjoint rater sets, train rows permuted); the chosen
    ones are queried by the user without ratings: the related list is exactly the item's list,
    and an item's query depends on its own raters' parameters only.  Per case of TIE_SPECS, on
    the first unused item where it works: with `top` the oracle's arg-max position (or its
    runner-up), the rater at list position `other` becomes top's copy -- the same embedding
    row(s), bias and rating -- and, if the two are then the list's top two (copy_pair_ok), its
    twin: MF: the bias one float32 ulp up or down; NCF: one gmf coordinate one ulp up or down.
    The first (item, top, step, coordinate) for which the recomputed oracle passes top_pair_ok
    with the fp64-larger key on the wanted side is taken; the exact cases keep the copy, at a
    position below / above top.  The choice reads the oracle only.
    Returns U, I, train, params, qu, qi, cases [(top, other, step)], the oracle results."""
    from oracle import fia_oracle as fo
    U, I = TIE_POOL * TIE_N + 1, TIE_POOL
    rng = np.random.default_rng(60)
    tu = np.concatenate([c * TIE_N + rng.permutation(TIE_N) for c in range(I)]).astype(np.int32)
    ti = np.repeat(np.arange(I), TIE_N).astype(np.int32)
    perm = rng.permutation(tu.size)
    tu, ti = tu[perm], ti[perm]
    tr = rng.integers(1, 6, tu.size).astype(np.float32)
    p = {name: a.copy() for name, a in params_for(model, U, I, k, TIE_SEED).items()}
    emb = ["embedding_layer/embedding_users"] if model == "MF" else \
        ["embedding_layer/mlp/embedding_users", "embedding_layer/gmf/embedding_users"]
    stepped = "embedding_layer/bias_users" if model == "MF" else emb[1]

    def influence_of(item):
        return fo.CsrExact(model, p, k, tu, ti, tr, WD, DAMPING).query(U - 1, item)["influence"]

    def build(item, spec):
        """The case on this item, or None (the item is left as it was)."""
        rows = np.nonzero(ti == item)[0]               # the item's list in index order
        saved_p, saved_tr = {name: a.copy() for name, a in p.items()}, tr.copy()
        for top in (int(t) for t in fo.topk(influence_of(item), 2)):
            other = {"below": top // 2, "above": (top + TIE_N) // 2}.get(spec[0], spec[0])
            if other == top:
                continue
            ut, uo = int(tu[rows[top]]), int(tu[rows[other]])
            tr[rows[other]] = tr[rows[top]]
            for name in emb:
                p[name].reshape(U, k)[uo] = p[name].reshape(U, k)[ut]
            if model == "MF":
                p[stepped][uo] = p[stepped][ut]
            if copy_pair_ok(influence_of(item), top, other):
                if spec[1] is None:
                    return top, other, 0
                for step in (+1, -1):
                    for at in ([uo] if model == "MF" else range(uo * k, uo * k + k)):
                        copied = p[stepped][at]
                        p[stepped][at] = np.nextafter(copied, np.float32(step * np.inf))
                        infl = influence_of(item)
                        if top_pair_ok(infl, top, other) and (fo.topk(infl, 1)[0] == min(top, other)) == spec[1]:
                            return top, other, step
                        p[stepped][at] = copied
            for name in p:
                p[name][...] = saved_p[name]
            tr[...] = saved_tr
        return None

    free = list(range(I))
    cases, items = [], []
    for spec in TIE_SPECS:
        for item in free:
            case = build(item, spec)
            if case:
                break
        else:
            raise AssertionError("no tie construction for case %r of %s k=%d" % (spec, model, k))
        free.remove(item)
        cases.append(case)
        items.append(item)
    qu = np.full(len(items), U - 1, np.int32)
    qi = np.array(items, np.int32)
    train = (tu, ti, tr)
    want = oracle_results(("ties", model, k), model, k, p, train, qu, qi)
    return U, I, train, p, qu, qi, cases, want


def assert_tie_preconditions(train, qi, cases, want):
    """On the oracle's values: every twin case passes top_pair_ok, and for each twin position
    the fp64-larger key sits once at the lower and once at the higher list position; the exact
    copies are the top two, (near) equal, with rank 3 clearly below.  Returns the expected
    top-1 position per case."""
    from oracle import fia_oracle as fo
    tu, ti, _ = train
    best, lower_wins = [], {}
    for c, (top, other, step) in enumerate(cases):
        infl = want[c]["influence"]
        assert np.array_equal(want[c]["rel"], np.nonzero(ti == qi[c])[0]) and infl.size == TIE_N
        first = fo.topk(infl, 3)
        if step:
            assert top_pair_ok(infl, top, other), (c, top, other, infl[top], infl[other])
            best.append(int(first[0]))
            lower_wins.setdefault(other, set()).add(int(first[0]) == min(top, other))
        else:
            assert copy_pair_ok(infl, top, other), (c, top, other, infl[top], infl[other])
            best.append(min(top, other))
    assert all(v == {True, False} for v in lower_wins.values()) and sorted(lower_wins) == sorted(TIE_OTHERS)
    below, above = cases[-2], cases[-1]
    assert below[1] < below[0] and above[1] > above[0]
    return best


@pytest.mark.parametrize("size", SIZES, ids=size_id)
def test_top1_f32_ties(size, tmp_path):
    """wave_top1_fast reduces the keys rounded to f32 and resolves exactly only when several
    lanes hold the f32 maximum.  Lists whose two largest |influence| are equal in f32 and differ
    by ~1e-9 relative in fp64 (far above NEAR_TIE and the kernels' ~1e-13): the twin in another
    lane of the same chunk (3), across the lane rows (70), at the chunk's last entry (127) and
    in the next chunk (128: the merge kernel's decision), the fp64-larger key once at the lower
    and once at the higher position; and bit-identical copies, where the lower position wins.
    K = 1 (the fast path) and K = 4 (the exact path): topk_pos[0] is the oracle's arg-max and
    topk_val carries that entry's bits."""
    model, k = size
    U, I, train, p, qu, qi, cases, want = tie_problem(model, k)
    best = assert_tie_preconditions(train, qi, cases, want)
    m = make_model(model, U, I, k, train, (qu, qi), p, tmpdir=tmp_path)
    for K in (1, 4):
        res = m.get_influence_batch(list(range(qu.size)), K=K)
        check_against_oracle(res, want, K, "f32 ties %s k=%d K=%d" % (model, k, K))
        for c, (top, other, step) in enumerate(cases):
            b, e = res["offsets"][c], res["offsets"][c + 1]
            infl = res["influence"][b:e]
            check_topk(res["topk_pos"][c], infl, want[c]["influence"], K)
            assert res["topk_pos"][c][0] == best[c], (K, c, top, other, step, res["topk_pos"][c])
            assert res["topk_idx"][c][0] == res["rel_idx"][b:e][best[c]], (K, c)
            assert bits(res["topk_val"][c][:1])[0] == bits(infl[best[c]:best[c] + 1])[0], (K, c)
            if not step:
                assert bits(infl[top:top + 1])[0] == bits(infl[other:other + 1])[0], (K, c, infl[top], infl[other])
    m.ctx.close()


NAN_LISTS = [(129, 5), (65, 10), (1, 0), (40, 17)]      # (raters, list position of the NaN-bias rater)


@pytest.mark.parametrize("k", [8, 16])
def test_top1_f32_ties_nan_key(k, tmp_path):
    """MF: an item's Gram does not read its raters' biases, so a rater whose bias_users entry is
    NaN gives exactly one NaN influence (asserted on the oracle) and a finite x.  Its key ranks
    last among the real entries: top-1 of a 129-list never returns its position, K = 64 on a
    65-list returns the 64 finite entries, K = 64 on a 40-list lists it last, before the unused
    slots, and top-1 of a one-rating list returns position 0 with a NaN value, not -1.
    Positions are compared directly (check_topk's tolerances are not NaN-safe)."""
    from oracle import fia_oracle as fo
    rng = np.random.default_rng(61)
    sizes = [n for n, _ in NAN_LISTS]
    U, I = sum(sizes) + 1, len(sizes)
    tu = rng.permutation(U - 1).astype(np.int32)
    ti = np.repeat(np.arange(I), sizes).astype(np.int32)
    perm = rng.permutation(tu.size)
    tu, ti = tu[perm], ti[perm]
    tr = rng.integers(1, 6, tu.size).astype(np.float32)
    p = {name: a.copy() for name, a in synth.mf_params(U, I, k, 6).items()}
    for c, (n, pos) in enumerate(NAN_LISTS):
        p["embedding_layer/bias_users"][tu[np.nonzero(ti == c)[0][pos]]] = np.nan
    qu = np.full(I, U - 1, np.int32)
    qi = np.arange(I, dtype=np.int32)
    want = oracle_results(("nan", k), "MF", k, p, (tu, ti, tr), qu, qi)
    order = []
    for c, (n, pos) in enumerate(NAN_LISTS):
        infl = want[c]["influence"]
        assert infl.size == n and np.array_equal(np.nonzero(np.isnan(infl))[0], [pos]) and np.isfinite(want[c]["x"]).all()
        a = np.sort(np.abs(infl[np.isfinite(infl)]))
        assert a.size < 2 or np.diff(a).min() > 1e-9 * a[-1]         # the finite entries' ranking is unambiguous
        order.append(fo.topk(infl, n))
        assert order[c][-1] == pos                                   # the oracle's rule: NaN last
    m = make_model("MF", U, I, k, (tu, ti, tr), (qu, qi), p, tmpdir=tmp_path)
    worst_i = worst_x = 0.0
    for K in (1, 4, 64):
        res = m.get_influence_batch(list(range(I)), K=K)
        for c, (n, pos) in enumerate(NAN_LISTS):
            b, e = res["offsets"][c], res["offsets"][c + 1]
            rel, infl = res["rel_idx"][b:e], res["influence"][b:e]
            assert np.array_equal(rel, want[c]["rel"])
            assert np.array_equal(np.nonzero(np.isnan(infl))[0], [pos]), (K, c)
            ok = np.isfinite(infl)
            if ok.any():
                worst_i = max(worst_i, rel_err(infl[ok], want[c]["influence"][ok]))
            worst_x = max(worst_x, rel_err(res["x"][c], want[c]["x"]))
            assert worst_i < RTOL and worst_x < RTOL, (K, c)
            got = res["topk_pos"][c]
            real = min(K, n)
            assert np.array_equal(got[:real], order[c][:real]), (K, c, got)
            assert (got[real:] == -1).all() and (res["topk_idx"][c][real:] == -1).all(), (K, c)
            assert np.array_equal(res["topk_idx"][c][:real], rel[got[:real]]), (K, c)
            assert np.array_equal(bits(res["topk_val"][c][:real]), bits(infl[got[:real]])), (K, c)
            assert np.isnan(res["topk_val"][c][real:]).all(), (K, c)
            if n > K:
                assert pos not in got, (K, c, got)
            else:
                assert got[n - 1] == pos and np.isnan(res["topk_val"][c][n - 1]), (K, c, got)
    print("nan key MF k=%d: %d queries x 3 K vs oracle, worst influence %.2e, worst x %.2e, 0 near-tie swaps"
          % (k, I, worst_i, worst_x))
    m.ctx.close()


# ---------------------------------------------------------------------------------------
# 5. a given inverse HVP at the same edges
# ---------------------------------------------------------------------------------------
def batch_x(m, qu, qi, x, K):
    """fia_query_batch_x through influence._lib (as RawModel.batch, with the given x [Q, D])."""
    t = m.torch
    dqu, dqi = m.dev_queries(qu, qi)
    off, tot = m.ctx.count_related(dqu, dqi)
    Q = len(qu)
    xin = t.from_numpy(np.ascontiguousarray(x, np.float64).reshape(-1)).to(m.dev)
    rel = t.full((max(tot, 1),), -7, dtype=t.int32, device=m.dev)
    infl = t.full((max(tot, 1),), float("nan"), dtype=t.float64, device=m.dev)
    tp = t.zeros(max(Q * K, 1), dtype=t.int64, device=m.dev)
    tix = t.zeros(max(Q * K, 1), dtype=t.int64, device=m.dev)
    tv = t.zeros(max(Q * K, 1), dtype=t.float64, device=m.dev)
    m.ctx.query_batch_x(dqu, dqi, off, tot, xin, rel, infl, K, tp, tix, tv)
    t.cuda.synchronize(m.dev)
    return dict(offsets=off.cpu().numpy(), rel_idx=rel[:tot].cpu().numpy().astype(np.int64),
                influence=infl[:tot].cpu().numpy(), topk_pos=tp.cpu().numpy().reshape(Q, K),
                topk_idx=tix.cpu().numpy().reshape(Q, K), topk_val=tv.cpu().numpy().reshape(Q, K))


@pytest.mark.parametrize("size", SIZES, ids=size_id)
def test_query_batch_x_on_edges(size):
    """fia_query_batch_x on the list-length problem (item lists), fed fia_query_batch's own
    x_out: k_record_x builds the record words (dup id, x . v, r-hat) these kernels consume, the
    batch holding the dup queries at list positions 0, 63, 64, 127, 128 and the lists' ends.
    Against the solve's own run: the same related lists, influence within 1e-12 relative per
    query (k_record_x sums x . theta and x . v in another order than the solve kernels; the
    bound of test_cached_inverse_hvp_force_refresh_false), top-1 positions equal wherever the
    oracle's top two differ by more than 1e-9 relative; a doubled x gives exactly doubled
    influence (bitwise)."""
    model, k = size
    K = 1
    U, I, train, qu, qi, dups, empty = edge_problem(1)
    p = params_for(model, U, I, k, 3)
    want = oracle_results(("edge", model, k, 1), model, k, p, train, qu, qi)
    assert_dup_positions(train, qu, qi, dups, want, 1)
    m = RawModel(model, k, U, I, train, p)
    first = m.batch(qu, qi, K)
    worst_i, worst_x, swaps = check_against_oracle(first, want, K, "solve run %s k=%d" % (model, k))
    again = batch_x(m, qu, qi, first["x"], K)
    twice = batch_x(m, qu, qi, 2.0 * first["x"], K)
    assert np.array_equal(again["offsets"], first["offsets"])
    assert np.array_equal(again["rel_idx"], first["rel_idx"]) and np.array_equal(twice["rel_idx"], first["rel_idx"])
    assert np.array_equal(bits(twice["influence"]), bits(2.0 * again["influence"]))
    offs = first["offsets"]
    worst, compared = 0.0, 0
    for q, o in enumerate(want):
        b, e = offs[q], offs[q + 1]
        if e == b:
            assert again["topk_pos"][q][0] == -1
            continue
        a, f = again["influence"][b:e], first["influence"][b:e]
        err = np.abs(a - f).max() / np.abs(f).max()
        assert err <= 1e-12, (q, err)
        worst = max(worst, err)
        top = np.sort(np.abs(o["influence"]))[::-1]
        if top.size < 2 or top[0] - top[1] > 1e-9 * top[0]:
            assert again["topk_pos"][q][0] == first["topk_pos"][q][0], q
            compared += 1
        pos = again["topk_pos"][q][0]
        assert again["topk_idx"][q][0] == again["rel_idx"][b:e][pos]
        assert bits(again["topk_val"][q])[0] == bits(a[pos:pos + 1])[0]
    assert compared > len(want) // 2
    print("given x %s k=%d: %d queries vs the solve's run, worst influence %.2e (solve run vs oracle: "
          "influence %.2e, x %.2e, %d near-tie swaps), %d top-1 positions compared"
          % (model, k, len(want), worst, worst_i, worst_x, swaps, compared))
    m.close()
