"""Oracle tests of the MF k in {32, 64} matrix-core scoring kernel (k_score_mf_mfma: every
query of those sizes with top-K <= 1, the reference single-query API among them) at the
shapes its index arithmetic depends on -- the 16-rating tile, the 3-slot row ring, the
64-entry list block, the 12-tile trip, the 256-rating chunk, the 4-chunk work item, the
four 16-query blocks of a workgroup and the rotated "aligned segment" stores -- plus the
NULL-output contract of every scoring kernel and the batch bound of the 32-bit offsets.

Every comparison is against the fp64 oracle (oracle.fia_oracle) unless it says bitwise:
related sets bit-exact, influence and x < RTOL (normalised as rel_err does), top-K by
check_topk.  All problems: wd = 1e-3, damping = 1e-6, parameters from synth.mf_params."""
import numpy as np
import pytest

from influence import synth
from test_gpu_parity import NEAR_TIE, RTOL, check_topk, make_model, rel_err

pytestmark = pytest.mark.gpu

WD, DAMPING = 1e-3, 1e-6
KS = [32, 64]


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def check_against_oracle(res, oracle_results, K, tag):
    """One batch result (the facade's dict) against the oracle's per-query results.  Returns
    (worst influence error, worst x error, near-tie swaps)."""
    offs = res["offsets"]
    assert offs[0] == 0 and offs.size == len(oracle_results) + 1
    worst_i = worst_x = 0.0
    swaps = 0
    for q, o in enumerate(oracle_results):
        b, e = offs[q], offs[q + 1]
        assert e - b == o["n"], (tag, q)
        rel, infl = res["rel_idx"][b:e], res["influence"][b:e]
        assert np.array_equal(rel, o["rel"]), (tag, q)
        if o["n"]:
            ei, ex = rel_err(infl, o["influence"]), rel_err(res["x"][q], o["x"])
            assert ei < RTOL and ex < RTOL, (tag, q, ei, ex)
            worst_i, worst_x = max(worst_i, ei), max(worst_x, ex)
        else:
            assert np.isnan(res["x"][q]).all(), (tag, q)
        if K:
            got = res["topk_pos"][q]
            swaps += check_topk(got, infl, o["influence"], K)
            want = got[got >= 0]
            assert want.size == min(K, o["n"]), (tag, q)
            assert np.array_equal(res["topk_idx"][q][:want.size], rel[want]), (tag, q)
            assert (res["topk_idx"][q][want.size:] == -1).all(), (tag, q)
            assert np.array_equal(bits(res["topk_val"][q][:want.size]), bits(infl[want])), (tag, q)
            assert np.isnan(res["topk_val"][q][want.size:]).all(), (tag, q)
    print("%s: %d queries vs oracle, worst influence %.2e, worst x %.2e, %d near-tie swaps"
          % (tag, len(oracle_results), worst_i, worst_x, swaps))
    return worst_i, worst_x, swaps


_ORACLE_CACHE = {}


def oracle_results(key, k, p, train, qu, qi):
    """CsrExact results of every query, computed once per problem and shared (read-only)."""
    from oracle import fia_oracle as fo
    if key not in _ORACLE_CACHE:
        tu, ti, tr = train
        ex = fo.CsrExact("MF", p, k, tu, ti, tr, WD, DAMPING)
        _ORACLE_CACHE[key] = [ex.query(int(u), int(i)) for u, i in zip(qu, qi)]
    return _ORACLE_CACHE[key]


# ---------------------------------------------------------------------------------------
# 1. list-length edges
# ---------------------------------------------------------------------------------------
LENGTHS = [1, 15, 16, 17, 47, 48, 49, 63, 64, 65, 191, 192, 193, 255, 256, 257, 1023, 1024, 1025]
# default_rng(EDGE_SEED): the long side's run starts cover all 16 residues mod 16 on both the
# item-side and the transposed (user-side) problem (asserted by the tests from the offsets)
EDGE_SEED = 32


def edge_problem(side, dup=False):
    """One long-list entity per length in LENGTHS (side 1: items hold them; side 0: the
    transposed problem, users hold them), the train rows permuted so that list order is
    train-row order and not id order.  Q = 59: per list a rater (its pair is a train row:
    coupled solve, the kernel's dup branch), a non-rater with a non-empty list and the
    entity with no ratings; one query on the unrated list; one with n_q = 0.
    dup: the 257-list is 256 distinct raters + the first rater's row once more."""
    rng = np.random.default_rng(EDGE_SEED)
    U, I = 1100, len(LENGTHS) + 1
    raters = []
    for n in LENGTHS:
        r = rng.choice(U - 1, n, replace=False).astype(np.int32)
        if dup and n == 257:
            r[-1] = r[0]
        raters.append(r)
    tu = np.concatenate(raters)
    ti = np.concatenate([np.full(r.size, j, np.int32) for j, r in enumerate(raters)])
    N = tu.size
    perm = rng.permutation(N)
    tu, ti = tu[perm], ti[perm]
    tr = rng.integers(1, 6, N).astype(np.float32)
    deg_u = np.bincount(tu, minlength=U)
    qs = []
    for j, r in enumerate(raters):
        others = np.setdiff1d(np.nonzero(deg_u > 0)[0], r)
        assert others.size > 0
        qs += [(int(r[0]), j), (int(rng.choice(others)), j), (U - 1, j)]
    qs += [(int(raters[5][0]), I - 1), (U - 1, I - 1)]
    qu = np.array([q[0] for q in qs], np.int32)
    qi = np.array([q[1] for q in qs], np.int32)
    assert N == 4801 and qu.size == 59
    if side == 0:
        U, I, tu, ti, qu, qi = I, U, ti, tu, qi, qu
    return U, I, (tu, ti, tr), qu, qi


def long_run_residues(offsets, train, U, I, qu, qi, side):
    """(first output element of the long side's run) % 16 over the queries whose list on that
    side has >= 17 entries: the rotation dl of the kernel's aligned-segment stores."""
    tu, ti, _ = train
    deg_u, deg_i = np.bincount(tu, minlength=U), np.bincount(ti, minlength=I)
    start = offsets[:-1] + (deg_u[qu] if side == 1 else 0)
    length = deg_i[qi] if side == 1 else deg_u[qu]
    return set(int(v) for v in start[length >= 17] % 16)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("side", [1, 0], ids=["item-lists", "user-lists"])
@pytest.mark.parametrize("K", [0, 1])
def test_list_length_edges(k, side, K, tmp_path):
    """Lists of every length at and beside the kernel's periods (tile 16, row ring 48, list
    block 64, 12-tile trip 192, chunk 256, work item 1024 -- 1025 is a second work item of one
    rating), on the item side and, transposed, on the user side; K = 0 (the single-query API's
    path) and K = 1.  The long side's runs start at every residue mod 16."""
    U, I, train, qu, qi = edge_problem(side)
    p = synth.mf_params(U, I, k, 3)
    m = make_model("MF", U, I, k, train, (qu, qi), p, tmpdir=tmp_path)
    res = m.get_influence_batch(list(range(qu.size)), K=K)
    residues = long_run_residues(res["offsets"], train, U, I, qu, qi, side)
    assert residues == set(range(16)), sorted(residues)
    want = oracle_results(("edge", k, side, False), k, p, train, qu, qi)
    assert want[-1]["n"] == 0 and res["offsets"][-1] == res["offsets"][-2]
    check_against_oracle(res, want, K, "edges k=%d side=%d K=%d" % (k, side, K))
    m.ctx.close()


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("K", [0, 1])
def test_list_length_edges_pair_twice_in_train(k, K, tmp_path):
    """The 257-list holds its first rater's row twice (the chunk's last entry is the second
    copy): that pair is in train twice, the coupled solve sums both residuals and each of the
    four related entries takes the dup branch; the copies of a train row carry identical bits."""
    U, I, train, qu, qi = edge_problem(1, dup=True)
    tu, ti, _ = train
    j = LENGTHS.index(257)
    q = 3 * j
    assert ((tu == qu[q]) & (ti == qi[q])).sum() == 2
    p = synth.mf_params(U, I, k, 3)
    m = make_model("MF", U, I, k, train, (qu, qi), p, tmpdir=tmp_path)
    res = m.get_influence_batch(list(range(qu.size)), K=K)
    want = oracle_results(("edge", k, 1, True), k, p, train, qu, qi)
    check_against_oracle(res, want, K, "edges+dup k=%d K=%d" % (k, K))
    b, e = res["offsets"][q], res["offsets"][q + 1]
    rel, infl = res["rel_idx"][b:e], res["influence"][b:e]
    twice = np.unique(rel[np.bincount(rel)[rel] > 1])
    assert twice.size == 2                       # both (u, i) rows, each in the user and the item list
    for row in twice:
        assert (rel == row).sum() == 2
        assert (bits(infl[rel == row]) == bits(infl[rel == row])[0]).all()
    m.ctx.close()


# ---------------------------------------------------------------------------------------
# 2. query-group sizes
# ---------------------------------------------------------------------------------------
GROUPS = [1, 15, 16, 17, 63, 64, 65, 130]


def group_problem():
    """Item j < 8 has about 300 ratings (two chunks, one work item) and is queried by
    GROUPS[j] distinct users: a partial block, blocks left empty (fetch-only waves), one full
    workgroup group of 64, a second group of one query, three groups.  User 0 is in 20 queries
    (a user-side group of more than one block) on 20 short-list items; one query is repeated."""
    rng = np.random.default_rng(21)
    U, I = 600, len(GROUPS) + 20
    us, its = [], []
    for j in range(len(GROUPS)):
        r = rng.choice(U, 290 + 3 * j, replace=False)
        us.append(r)
        its.append(np.full(r.size, j))
    for j in range(len(GROUPS), I):
        r = rng.choice(U, 6 + j % 5, replace=False)
        us.append(r)
        its.append(np.full(r.size, j))
    tu = np.concatenate(us).astype(np.int32)
    ti = np.concatenate(its).astype(np.int32)
    perm = rng.permutation(tu.size)
    tu, ti = tu[perm], ti[perm]
    tr = rng.integers(1, 6, tu.size).astype(np.float32)
    qs = []
    for j, g in enumerate(GROUPS):
        qs += [(int(u), j) for u in rng.choice(np.arange(1, U), g, replace=False)]
    qs += [(0, j) for j in range(len(GROUPS), I)]
    qs.append(qs[sum(GROUPS) - 1])                # the repeated query: in the group of 130
    order = rng.permutation(len(qs))
    qu = np.array([qs[t][0] for t in order], np.int32)
    qi = np.array([qs[t][1] for t in order], np.int32)
    return U, I, (tu, ti, tr), qu, qi


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("K", [0, 1])
def test_query_group_sizes(k, K, tmp_path):
    """Entity groups of 1, 15, 16, 17, 63, 64, 65 and 131 queries on two-chunk lists, a user in
    20 queries and a repeated query, in shuffled batch order: every query against CsrExact."""
    U, I, train, qu, qi = group_problem()
    per_item = np.bincount(qi, minlength=I)
    assert list(per_item[:len(GROUPS)]) == GROUPS[:-1] + [GROUPS[-1] + 1]    # (+ the repeated query)
    assert np.bincount(qu, minlength=U)[0] == 20
    pairs = qu.astype(np.int64) * I + qi
    assert np.unique(pairs).size == pairs.size - 1
    p = synth.mf_params(U, I, k, 4)
    m = make_model("MF", U, I, k, train, (qu, qi), p, tmpdir=tmp_path)
    res = m.get_influence_batch(list(range(qu.size)), K=K)
    want = oracle_results(("groups", k), k, p, train, qu, qi)
    check_against_oracle(res, want, K, "groups k=%d K=%d" % (k, K))
    m.ctx.close()


# ---------------------------------------------------------------------------------------
# 3. a long list and the top-K merge kernel that reads this kernel's candidates
# ---------------------------------------------------------------------------------------
def long_problem():
    rng = np.random.default_rng(33)
    U, I, N = 2600, 30, 3000
    key = np.sort(rng.choice((U - 1) * (I - 1), N, replace=False))
    tu, ti = (key // (I - 1)).astype(np.int32), (key % (I - 1)).astype(np.int32)
    ex = rng.choice(U - 1, 2100, replace=False).astype(np.int32)     # item I-1: 2100 raters
    tu = np.concatenate([tu, ex]).astype(np.int32)
    ti = np.concatenate([ti, np.full(ex.size, I - 1, np.int32)]).astype(np.int32)
    perm = rng.permutation(tu.size)
    tu, ti = tu[perm], ti[perm]
    tr = rng.integers(1, 6, tu.size).astype(np.float32)
    non_rater = int(np.setdiff1d(np.arange(U - 1), ex)[0])
    long_qs = [(int(ex[0]), I - 1), (non_rater, I - 1), (U - 1, I - 1)]
    short_qs = [(int(u), int(i)) for u, i in zip(rng.integers(0, U - 1, 12), rng.integers(0, I - 1, 12))]
    return U, I, (tu, ti, tr), long_qs, short_qs


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("merge", ["wave", "thread"])
def test_long_list_top1_through_both_merge_kernels(k, merge, tmp_path):
    """An item of 2100 raters: three work items (1024 + 1024 + 52), candidate slots
    cg * 4 + chunk over nine chunks.  The merge kernel is chosen by
    max_chunks = 2 Q + total_rel / 128 + 1 <= 16 Q (K <= 4):
      wave:   Q = 3,  total ~ 6.3k:  6 + 49 + 1 = 56  > 48   -> k_topk_merge (wave per query)
      thread: Q = 15, total ~ 7.6k: 30 + 59 + 1 = 90 <= 240  -> k_topk_merge_thread
    (asserted below from the batch's own Q and total).  Top-1 position, train row and value
    against the oracle in both."""
    from oracle import fia_oracle as fo
    U, I, train, long_qs, short_qs = long_problem()
    qs = long_qs + (short_qs if merge == "thread" else [])
    qu = np.array([q[0] for q in qs], np.int32)
    qi = np.array([q[1] for q in qs], np.int32)
    p = synth.mf_params(U, I, k, 5)
    m = make_model("MF", U, I, k, train, (qu, qi), p, tmpdir=tmp_path)
    res = m.get_influence_batch(list(range(qu.size)), K=1)
    Q, total = qu.size, int(res["offsets"][-1])
    max_chunks = 2 * Q + total // 128 + 1
    assert (max_chunks > 16 * Q) == (merge == "wave"), (Q, total, max_chunks)
    want = oracle_results(("long", k, merge), k, p, train, qu, qi)
    assert all(o["n"] >= 2100 for o in want[:3])
    check_against_oracle(res, want, 1, "long k=%d %s-merge" % (k, merge))
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
# the C ABI driven directly (sections 4, 6, 7)
# ---------------------------------------------------------------------------------------
class RawModel(object):
    """A fia context set up through influence._lib alone (the facade's constructor always
    runs a full fia_prepare; here the first prepare is the caller's)."""

    def __init__(self, model, k, U, I, train, params, prepare=True, wd=WD, damping=DAMPING):
        import torch
        from influence import _lib
        self.torch, self.lib = torch, _lib
        self.dev = torch.device("cuda:0")
        self.ctx = _lib.Context(0)
        self.tables = [torch.from_numpy(np.ascontiguousarray(params[n], np.float32)).to(self.dev) for n in params]
        self.ctx.set_params(_lib.FIA_MODEL_MF if model == "MF" else _lib.FIA_MODEL_NCF, k, U, I, self.tables,
                            wd, damping)
        tu, ti, tr = train
        self.train = [torch.from_numpy(np.ascontiguousarray(a, t)).to(self.dev)
                      for a, t in ((tu, np.int32), (ti, np.int32), (tr, np.float32))]
        self.ctx.build_index(self.train[0], self.train[1], self.train[2], U, I)
        if prepare:
            self.ctx.prepare()

    def dev_queries(self, qu, qi):
        t = self.torch
        return (t.from_numpy(np.ascontiguousarray(qu, np.int32)).to(self.dev),
                t.from_numpy(np.ascontiguousarray(qi, np.int32)).to(self.dev))

    def prepare_for(self, qu, qi):
        self.ctx.prepare_for(*self.dev_queries(qu, qi))

    def batch(self, qu, qi, K):
        """As GenericNeuralNet.get_influence_batch(full=True): count (checked), then query."""
        t = self.torch
        dqu, dqi = self.dev_queries(qu, qi)
        off, tot = self.ctx.count_related(dqu, dqi)
        Q, D = len(qu), self.ctx.num_params()
        rel = t.full((max(tot, 1),), -7, dtype=t.int32, device=self.dev)
        infl = t.full((max(tot, 1),), float("nan"), dtype=t.float64, device=self.dev)
        x = t.zeros(Q * D, dtype=t.float64, device=self.dev)
        tp = t.zeros(max(Q * K, 1), dtype=t.int64, device=self.dev) if K else None
        tix = t.zeros(max(Q * K, 1), dtype=t.int64, device=self.dev) if K else None
        tv = t.zeros(max(Q * K, 1), dtype=t.float64, device=self.dev) if K else None
        self.ctx.query_batch(dqu, dqi, off, tot, rel, infl, x, K, tp, tix, tv)
        t.cuda.synchronize(self.dev)
        out = dict(offsets=off.cpu().numpy(), rel_idx=rel[:tot].cpu().numpy().astype(np.int64),
                   influence=infl[:tot].cpu().numpy(), x=x.cpu().numpy().reshape(Q, D))
        if K:
            out.update(topk_pos=tp.cpu().numpy().reshape(Q, K), topk_idx=tix.cpu().numpy().reshape(Q, K),
                       topk_val=tv.cpu().numpy().reshape(Q, K))
        return out

    def close(self):
        self.ctx.close()


def dense_problem(seed, U, I, N):
    rng = np.random.default_rng(seed)
    key = np.sort(rng.choice(U * I, N, replace=False))
    tu, ti = (key // I).astype(np.int32), (key % I).astype(np.int32)
    tr = rng.integers(1, 6, N).astype(np.float32)
    return rng, (tu, ti, tr)


# ---------------------------------------------------------------------------------------
# 4. fia_prepare_for feeding the MFMA kernel
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("K", [0, 1])
def test_prepare_for_first_then_mfma_scoring(k, K):
    """A context whose FIRST prepare is fia_prepare_for: the Gram pass has written the
    list-ordered residuals of the marked entities only (the others were never written).  The
    subset -- 70 queries on one item (more than a workgroup group of 64), a train-pair query,
    a few more -- matches the oracle; after a full fia_prepare the same subset is bitwise the
    same; a query outside the subset is refused in between."""
    from influence._lib import FIAError
    U, I, N = 400, 12, 2500
    rng, train = dense_problem(50 + k, U, I, N)
    tu, ti, tr = train
    p = synth.mf_params(U, I, k, 9)
    marked_users = rng.choice(U, 90, replace=False)
    qs = [(int(u), 3) for u in marked_users[:70]] + [(int(tu[17]), int(ti[17]))] + \
         [(int(u), 7) for u in marked_users[70:80]] + [(int(u), 3) for u in marked_users[80:90]]
    qu = np.array([q[0] for q in qs], np.int32)
    qi = np.array([q[1] for q in qs], np.int32)
    assert (qi == 3).sum() > 64
    m = RawModel("MF", k, U, I, train, p, prepare=False)
    m.prepare_for(qu, qi)
    part = m.batch(qu, qi, K)
    want = oracle_results(("subset", k), k, p, train, qu, qi)
    check_against_oracle(part, want, K, "prepare_for k=%d K=%d" % (k, K))
    out_u = int(np.setdiff1d(np.arange(U), qu)[0])
    out_i = int(np.setdiff1d(np.arange(I), qi)[0])
    for u, i in ((out_u, 3), (int(qu[0]), out_i)):
        with pytest.raises(FIAError):
            m.batch(np.array([u], np.int32), np.array([i], np.int32), K)
    m.ctx.prepare()
    full = m.batch(qu, qi, K)
    for name in part:
        assert np.array_equal(part[name], full[name], equal_nan=True), name
    for name in ("influence", "x"):
        assert np.array_equal(bits(part[name]), bits(full[name])), name
    m.close()


# ---------------------------------------------------------------------------------------
# 5. the reference single-query API at k >= 32
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,k", [("MF", 32), ("MF", 64), ("NCF", 32), ("MF", 128), ("NCF", 64)])
def test_single_query_api_large_sizes(model, k, tmp_path):
    """test_small_golden_single_query_api's contract at the sizes it leaves out, on the problem
    of test_every_built_size_matches_oracle: the MF k = 32, 64 rows are the K = 0, one-query
    MFMA path (one live query row, three fetch-only waves)."""
    from oracle import fia_oracle as fo
    rng = np.random.default_rng(k + (100 if model == "NCF" else 0))
    U, I, N = 700, 30, 3000
    key = np.sort(rng.choice((U - 1) * I, N - 1, replace=False))
    tu, ti = (key // I).astype(np.int32), (key % I).astype(np.int32)
    extra_u = np.arange(U - 1, dtype=np.int32)
    tu = np.concatenate([tu, extra_u, [tu[5]]]).astype(np.int32)
    ti = np.concatenate([ti, np.full(U - 1, I - 1, np.int32), [ti[5]]]).astype(np.int32)
    tr = rng.integers(1, 6, tu.size).astype(np.float32)
    p = synth.mf_params(U, I, k, 3) if model == "MF" else synth.ncf_params(U, I, k, 3)
    qs = [(1, 2), (int(tu[5]), int(ti[5])), (U - 1, 3), (7, I - 1), (int(tu[50]), int(ti[50]))]
    qu = np.array([q[0] for q in qs], np.int32)
    qi = np.array([q[1] for q in qs], np.int32)
    m = make_model(model, U, I, k, (tu, ti, tr), (qu, qi), p, tmpdir=tmp_path)
    worst_i = worst_x = 0.0
    for q, (u, i) in enumerate(qs):
        o = fo.query(model, p, k, tu, ti, tr, u, i, WD, DAMPING)
        rel = m.get_train_indices_of_test_case([q])
        assert rel.dtype == np.int64 and np.array_equal(rel, o["rel"]), (model, k, q)
        infl = m.get_influence_on_test_loss([q], np.arange(tu.size))
        assert np.array_equal(m.train_indices_of_test_case, o["rel"]), (model, k, q)
        assert infl.dtype == np.float64 and infl.shape == (o["n"],)
        x = np.concatenate([np.ravel(a) for a in m.inverse_hvp])
        if o["n"]:
            ei, ex = rel_err(infl, o["influence"]), rel_err(x, o["x"])
            assert ei < RTOL and ex < RTOL, (model, k, q, ei, ex)
            worst_i, worst_x = max(worst_i, ei), max(worst_x, ex)
        else:
            assert np.isnan(x).all()
    print("single-query %s k=%d: worst influence %.2e, worst x %.2e" % (model, k, worst_i, worst_x))
    m.ctx.close()


# ---------------------------------------------------------------------------------------
# 6. NULL outputs and guard bands, every scoring kernel
# ---------------------------------------------------------------------------------------
SCORING_KERNELS = [
    ("MF", 8, 1), ("MF", 16, 1),                             # k_score_mf_runs
    ("NCF", 8, 1), ("NCF", 16, 1),                           # k_score_ncf_runs
    ("MF", 32, 0), ("MF", 32, 1), ("MF", 64, 0), ("MF", 64, 1),   # k_score_mf_mfma
    ("MF", 32, 2), ("MF", 64, 2),                            # k_score_grouped_mf
    ("NCF", 32, 1),                                          # k_score_ncf
    ("MF", 128, 1), ("NCF", 64, 1),                          # k_big_score_mfma
    ("MF", 256, 1), ("NCF", 128, 0), ("NCF", 256, 1),
]
GUARD = 64                       # sentinel elements on each side of an output (at least)
REL_SENTINEL = -7
INFL_SENTINEL = 1.2345678e300    # finite, and no influence of these problems is near it


@pytest.mark.parametrize("model,k,K", SCORING_KERNELS)
def test_null_outputs_and_guard_bands(model, k, K):
    """fia_query_batch lets rel_idx and influence be NULL independently.  Each output is a
    view buf[s : s + total] of a larger tensor of sentinels, s in {64, 65, 69} (the base is and
    is not 128-B aligned): nothing outside the view is written, everything inside is, an output
    that is given equals the both-outputs run bitwise whichever other output is NULL, the
    top-K arrays and x of all four runs are equal, and the both-outputs run matches the
    oracle on a sample of queries."""
    import torch
    from oracle import fia_oracle as fo
    U, I, N = 300, 40, 4000
    rng, train = dense_problem(61, U, I, N)
    tu, ti, tr = train
    p = synth.mf_params(U, I, k, 2) if model == "MF" else synth.ncf_params(U, I, k, 2)
    qi = rng.integers(0, I, 60).astype(np.int32)
    qu = rng.integers(0, U, 60).astype(np.int32)
    qu[30], qi[30] = tu[11], ti[11]                  # a train pair
    order = np.argsort(qi, kind="stable")            # sorted by item (the k <= 16 item runs)
    qu, qi = qu[order], qi[order]
    pair_q = int(np.nonzero(order == 30)[0][0])
    m = RawModel(model, k, U, I, train, p)
    dev = m.dev
    dqu, dqi = m.dev_queries(qu, qi)
    off, tot = m.ctx.count_related(dqu, dqi)
    offs = off.cpu().numpy()
    Q, D = qu.size, m.ctx.num_params()
    for s in (64, 65, 69):
        runs = {}
        for mode in ("both", "rel", "infl", "none"):
            relbuf = torch.full((s + tot + GUARD + 5,), REL_SENTINEL, dtype=torch.int32, device=dev)
            inflbuf = torch.full((s + tot + GUARD + 5,), INFL_SENTINEL, dtype=torch.float64, device=dev)
            rel = relbuf[s:s + tot] if mode in ("both", "rel") else None
            infl = inflbuf[s:s + tot] if mode in ("both", "infl") else None
            x = torch.zeros(Q * D, dtype=torch.float64, device=dev)
            tp = torch.full((Q * K,), -5, dtype=torch.int64, device=dev) if K else None
            tix = torch.full((Q * K,), -5, dtype=torch.int64, device=dev) if K else None
            tv = torch.zeros(Q * K, dtype=torch.float64, device=dev) if K else None
            m.ctx.query_batch(dqu, dqi, off, tot, rel, infl, x, K, tp, tix, tv)
            torch.cuda.synchronize(dev)
            r = dict(rel=relbuf.cpu().numpy(), infl=inflbuf.cpu().numpy(), x=x.cpu().numpy())
            if K:
                r.update(tp=tp.cpu().numpy(), tix=tix.cpu().numpy(), tv=tv.cpu().numpy())
            runs[mode] = r
            tag = (model, k, K, s, mode)
            # the guard bands (an output that was not given: its whole buffer)
            inside = np.zeros(relbuf.numel(), bool)
            inside[s:s + tot] = True
            rel_in = inside if rel is not None else np.zeros_like(inside)
            infl_in = inside if infl is not None else np.zeros_like(inside)
            assert (r["rel"][~rel_in] == REL_SENTINEL).all(), tag
            assert (r["infl"][~infl_in] == INFL_SENTINEL).all(), tag
            assert (r["rel"][rel_in] != REL_SENTINEL).all(), tag
            assert (r["infl"][infl_in] != INFL_SENTINEL).all(), tag
        both = runs["both"]
        for mode in ("rel", "infl", "none"):
            r = runs[mode]
            if mode == "rel":
                assert np.array_equal(r["rel"], both["rel"]), (model, k, K, s, mode)
            if mode == "infl":
                assert np.array_equal(bits(r["infl"]), bits(both["infl"])), (model, k, K, s, mode)
            assert np.array_equal(bits(r["x"]), bits(both["x"])), (model, k, K, s, mode)
            if K:
                assert np.array_equal(r["tp"], both["tp"]), (model, k, K, s, mode)
                assert np.array_equal(r["tix"], both["tix"]), (model, k, K, s, mode)
                assert np.array_equal(r["tv"], both["tv"], equal_nan=True), (model, k, K, s, mode)
        rel_all, infl_all = both["rel"][s:s + tot].astype(np.int64), both["infl"][s:s + tot]
        if s == 64:
            first = (rel_all, infl_all)
            worst = 0.0
            for q in sorted({0, 13, 47, 59, pair_q}):
                o = fo.query(model, p, k, tu, ti, tr, int(qu[q]), int(qi[q]), WD, DAMPING)
                b, e = offs[q], offs[q + 1]
                assert np.array_equal(rel_all[b:e], o["rel"]), (model, k, K, q)
                err = rel_err(infl_all[b:e], o["influence"])
                assert err < RTOL and rel_err(both["x"].reshape(Q, D)[q], o["x"]) < RTOL, (model, k, K, q)
                worst = max(worst, err)
                if K:
                    got = both["tp"].reshape(Q, K)[q]
                    check_topk(got, infl_all[b:e], o["influence"], K)
                    pos = got[got >= 0]
                    assert np.array_equal(both["tix"].reshape(Q, K)[q][:pos.size], rel_all[b:e][pos]), (model, k, K, q)
                    assert np.array_equal(bits(both["tv"].reshape(Q, K)[q][:pos.size]), bits(infl_all[b:e][pos])), \
                        (model, k, K, q)
            print("null-outputs %s k=%d K=%d: worst influence %.2e on the sample" % (model, k, K, worst))
        else:
            # the same batch at another base offset: the same bits
            assert np.array_equal(rel_all, first[0]) and np.array_equal(bits(infl_all), bits(first[1])), (model, k, K, s)
    m.close()


# ---------------------------------------------------------------------------------------
# 7. the batch bound of the MFMA path's 32-bit offsets
# ---------------------------------------------------------------------------------------
def test_mfma_batch_bound_enforced():
    """MF k in {32, 64}, K <= 1: total_rel above 2^32 (the kernel's uint32 element offsets)
    is refused with FIA_ERR_INVALID before anything is reserved or launched (include/fia.h,
    fia_query_batch); the true total is accepted on the same context right after; the same
    total on MF k = 16 (64-bit offsets) is not refused."""
    import torch
    from influence._lib import FIAError
    U, I, N = 300, 40, 4000
    rng, train = dense_problem(70, U, I, N)
    qu = np.array([3, 200], np.int32)
    qi = np.array([5, 17], np.int32)
    first_rejected = (1 << 32) + 1
    for k in (64, 16):
        p = synth.mf_params(U, I, k, 2)
        m = RawModel("MF", k, U, I, train, p)
        want = m.batch(qu, qi, 0)
        dqu, dqi = m.dev_queries(qu, qi)
        off, tot = m.ctx.count_related(dqu, dqi)
        D = m.ctx.num_params()

        def lean(total, K=0):
            x = torch.zeros(2 * D, dtype=torch.float64, device=m.dev)
            tk = [torch.zeros(2 * K, dtype=t, device=m.dev) for t in (torch.int64, torch.int64, torch.float64)] \
                if K else [None] * 3
            m.ctx.query_batch(dqu, dqi, off, total, None, None, x, K, *tk)
            torch.cuda.synchronize(m.dev)
            return x.cpu().numpy().reshape(2, D)

        if k == 64:
            for K in (0, 1):
                with pytest.raises(FIAError, match="invalid argument"):
                    lean(first_rejected, K)
            assert np.array_equal(bits(lean(first_rejected - 1)), bits(want["x"]))   # the last accepted value
            assert np.array_equal(bits(lean(tot)), bits(want["x"]))
        else:
            assert np.array_equal(bits(lean(first_rejected)), bits(want["x"]))
        m.close()
