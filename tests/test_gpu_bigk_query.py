"""Oracle tests of the large-k query path (fia_query_batch / fia_query_batch_x at MF k in
{128, 256} and NCF k in {64, 128, 256}: bigk.hip and the kernel units bigk_prepare.hip,
bigk_solve.hip, bigk_solve_batched.hip, bigk_score.hip) at the shapes its index arithmetic
depends on -- the scorer's 16-rating tile, 64-rating pass and 256-rating chunk, its one-half
and two-half MFMA variants (more than 16 queries of one entity) and second query block (more
than 32), the Gram kernel's 16-rating slabs, 2048-rating slices and the combine of 2 and 3
partials, a zero-length Gram work item, the persistent loop of k_big_solve (more coupled
queries than resident workgroups), the system counts around the 8-wide k_bs_trail grid
rounding, k_big_record_x as a batch, the three top-K merge kernels fed from this path's four
candidates per chunk, and fia_prepare_for of a few entities at k = 256 (the XCD-ordered Gram
grid of NCF k = 256 with a work-item count that is no multiple of 8).

Every comparison is against the fp64 oracle (oracle.fia_oracle.CsrExact) unless it says
bitwise: related lists bit-exact, influence and x < RTOL (normalised as rel_err does), top-K
by check_topk, topk_idx = rel[pos], topk_val the bits of influence[pos], unused slots
-1 / NaN; rows that sit twice in a related list carry identical bits.  No query is left out
of a comparison it belongs to: a query without related ratings has x all NaN, as the oracle
says.  MF k = 128 and NCF k = 64 (D = 258 / 256) compare every query; the other three sizes
compare the sample each test names (an oracle solve there is up to 1024 x 1024) and, for
EVERY query, the related list, finite values and the top-K selection on the kernel's own values.

Device memory: a cached entity costs 1.08 MB of Gram at NCF k = 256 (0.3 MB at MF k = 256), so
the problems with thousands of entities (the list-length ladder, the query groups, the coupled
batch) call fia_prepare_for(queries) at MF 256 / NCF 128 / NCF 256 and a plain fia_prepare at
MF 128 / NCF 64; the 344-entity problem is prepared in full at every size.  List lengths are
exact because every id inside a list is distinct; they are asserted from np.bincount before
the GPU call.  All problems: wd = 1e-3, damping = 1e-6, parameters from synth.mf_params /
synth.ncf_params.

The kernel numbers a query inside its entity's group by atomic arrival (k_group_count), which
follows the batch order in practice but is not promised to: the tests place coupled queries by
batch order and assert nothing that depends on the rank a query ended up with."""
import functools

import numpy as np
import pytest

from influence import synth
from test_gpu_mfma_score import DAMPING, WD, RawModel, bits, check_against_oracle, dense_problem
from test_gpu_parity import RTOL, check_topk, make_model, rel_err

pytestmark = pytest.mark.gpu

SIZES = [("MF", 128), ("MF", 256), ("NCF", 64), ("NCF", 128), ("NCF", 256)]     # FIA_BIG_SIZES
SMALL = {("MF", 128), ("NCF", 64)}       # every query against the oracle, plain fia_prepare
BIG_SLICE = 2048                         # kBigSlice: ratings per Gram work item
CHUNK = 256                              # kChunk
RUN_CHUNK = 128                          # kRunChunk: the ABI's max_chunks = 2 Q + total / 128 + 1


def size_id(v):
    return "%s-%d" % v if isinstance(v, tuple) else None


@functools.lru_cache(maxsize=None)
def params_for(size, U, I, seed):
    model, k = size
    return synth.mf_params(U, I, k, seed) if model == "MF" else synth.ncf_params(U, I, k, seed)


_EXACT = {}
_MEMO = {}


def exact_for(key, size, p, train):
    """The CsrExact oracle of one (problem, size), built once."""
    from oracle import fia_oracle as fo
    if (key, size) not in _EXACT:
        tu, ti, tr = train
        _EXACT[(key, size)] = fo.CsrExact(size[0], p, size[1], tu, ti, tr, WD, DAMPING)
    return _EXACT[(key, size)]


def oracle_results(key, size, p, train, qu, qi):
    """CsrExact results of the given queries; a pair is solved once per (problem, size) and
    shared (read-only) by every test that asks for it.  Short lists keep G, e and theta too."""
    ex = exact_for(key, size, p, train)
    out = []
    for u, i in zip(qu, qi):
        mk = (key, size, int(u), int(i))
        if mk not in _MEMO:
            o = ex.query(int(u), int(i))
            names = ("rel", "n", "influence", "x") + (("G", "e", "theta") if 0 < o["n"] < 1000 else ())
            _MEMO[mk] = {name: o[name] for name in names}
        out.append(_MEMO[mk])
    return out


def prepare(m, size, qu, qi):
    if size in SMALL:
        m.ctx.prepare()
    else:
        m.prepare_for(qu, qi)


def take(res, idx):
    """The batch result restricted to the queries idx (in that order), offsets re-based."""
    offs = res["offsets"]
    idx = [int(q) for q in idx]
    lens = [int(offs[q + 1] - offs[q]) for q in idx]
    out = dict(offsets=np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), x=res["x"][idx])
    for name in ("rel_idx", "influence"):
        out[name] = np.concatenate([res[name][offs[q]:offs[q + 1]] for q in idx])
    for name in ("topk_pos", "topk_idx", "topk_val"):
        if name in res:
            out[name] = res[name][idx]
    return out


def check_lists(res, ex, qu, qi, K, tag):
    """EVERY query of a batch, without a solve: offsets, the related list bit-exact, finite
    influence and x (NaN x for an empty list), and the top-K arrays as the selection rule gives
    them on the kernel's own values."""
    from oracle import fia_oracle as fo
    offs = res["offsets"]
    assert offs[0] == 0 and offs.size == len(qu) + 1, tag
    for q in range(len(qu)):
        rel = ex.related(int(qu[q]), int(qi[q]))
        b, e = offs[q], offs[q + 1]
        assert np.array_equal(res["rel_idx"][b:e], rel), (tag, q)
        infl = res["influence"][b:e]
        assert np.isfinite(infl).all(), (tag, q)
        if e > b:
            assert np.isfinite(res["x"][q]).all(), (tag, q)
        else:
            assert np.isnan(res["x"][q]).all(), (tag, q)
        if K:
            want = fo.topk(infl, K)
            got = res["topk_pos"][q]
            assert np.array_equal(got[:want.size], want) and (got[want.size:] == -1).all(), (tag, q)
            assert np.array_equal(res["topk_idx"][q][:want.size], rel[want]), (tag, q)
            assert (res["topk_idx"][q][want.size:] == -1).all(), (tag, q)
            assert np.array_equal(bits(res["topk_val"][q][:want.size]), bits(infl[want])), (tag, q)
            assert np.isnan(res["topk_val"][q][want.size:]).all(), (tag, q)


def assert_dup_bits(res, q, tag):
    """The rows that sit twice in query q's related list (its own pair's train rows: once in
    the user list, once in the item list) carry identical bits.  Returns their number."""
    b, e = res["offsets"][q], res["offsets"][q + 1]
    rel, infl = res["rel_idx"][b:e], res["influence"][b:e]
    twice = np.unique(rel[np.bincount(rel)[rel] > 1])
    assert twice.size >= 1, (tag, q)
    for row in twice:
        v = bits(infl[rel == row])
        assert v.size == 2 and v[0] == v[1], (tag, q, row)
    return twice.size


def same_query_bits(ra, qa, rb, qb, K, tag):
    """Query qa of result ra and query qb of result rb: every output bit for bit."""
    ba, ea = ra["offsets"][qa], ra["offsets"][qa + 1]
    bb, eb = rb["offsets"][qb], rb["offsets"][qb + 1]
    assert ea - ba == eb - bb, tag
    assert np.array_equal(ra["rel_idx"][ba:ea], rb["rel_idx"][bb:eb]), tag
    assert np.array_equal(bits(ra["influence"][ba:ea]), bits(rb["influence"][bb:eb])), tag
    assert np.array_equal(bits(ra["x"][qa]), bits(rb["x"][qb])), tag
    if K:
        assert np.array_equal(ra["topk_pos"][qa], rb["topk_pos"][qb]), tag
        assert np.array_equal(ra["topk_idx"][qa], rb["topk_idx"][qb]), tag
        assert np.array_equal(bits(ra["topk_val"][qa]), bits(rb["topk_val"][qb])), tag


def gram_items(deg, entities):
    """Gram work items of the marked entities of one side (big_work_lists): one per started
    2048-rating slice, one for an empty list."""
    return int(sum(max(1, -(-int(deg[e]) // BIG_SLICE)) for e in set(int(e) for e in entities)))


# ---------------------------------------------------------------------------------------
# 1. list-length ladder
# ---------------------------------------------------------------------------------------
LADDER = [0, 1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 511, 512, 513, 2047, 2048, 2049, 4097]
LADDER_SAMPLE = {0, 1, 17, 65, 257, 513, 2049, 4097}      # compared at the three larger sizes, variants a and c
N_PARTNERS, N_FILLERS = 6, 8


@functools.lru_cache(maxsize=None)
def ladder_problem(side):
    """One entity per length of LADDER (side 1: items hold the lists; side 0: the transposed
    problem, users hold them, without the 4097-list so the item table stays small), its raters
    distinct ids of a pool, the train rows permuted so that list order is train-row order and
    not id order.  Every ladder entity is queried, in one batch, by (a) the partner without
    ratings, (b) a partner with a short list that has not rated it and, for lengths >= 1,
    (c) the partner of the LAST row of its list (a train pair: the coupled solve, the dup row in
    the partly filled last tile).  The other side's lists hold at most 20 ratings.
    Returns U, I, train, qu, qi, kinds [(length, variant)] per query."""
    lengths = LADDER if side == 1 else LADDER[:-1]
    rng = np.random.default_rng(71 + side)
    L, P = len(lengths), max(lengths) + 3
    U, I = P + N_PARTNERS + 1, L + N_FILLERS
    us = [rng.choice(P, n, replace=False) for n in lengths]
    its = [np.full(n, j) for j, n in enumerate(lengths)]
    for f in range(N_FILLERS):                       # the (b) partners' short lists
        r = np.concatenate([P + (f + np.arange(3)) % N_PARTNERS, rng.choice(P, 5, replace=False)])
        us.append(r)
        its.append(np.full(r.size, L + f))
    tu, ti = np.concatenate(us).astype(np.int32), np.concatenate(its).astype(np.int32)
    perm = rng.permutation(tu.size)
    tu, ti = tu[perm], ti[perm]
    tr = rng.integers(1, 6, tu.size).astype(np.float32)
    deg_u, deg_i = np.bincount(tu, minlength=U), np.bincount(ti, minlength=I)
    assert list(deg_i[:L]) == lengths and deg_u.max() <= 20 and deg_u[U - 1] == 0
    assert (deg_u[P:P + N_PARTNERS] > 0).all()
    qs, kinds = [], []
    for j, n in enumerate(lengths):
        qs += [(U - 1, j), (P + j % N_PARTNERS, j)]
        kinds += [(n, "a"), (n, "b")]
        if n:
            last = int(np.nonzero(ti == j)[0][-1])           # the list's last entry: its last train row
            assert ((tu == tu[last]) & (ti == j)).sum() == 1
            qs.append((int(tu[last]), j))
            kinds.append((n, "c"))
    qu = np.array([q[0] for q in qs], np.int32)
    qi = np.array([q[1] for q in qs], np.int32)
    if side == 0:
        U, I, tu, ti, qu, qi = I, U, ti, tu, qi, qu
    return U, I, (tu, ti, tr), qu, qi, tuple(kinds)


@pytest.mark.parametrize("size", SIZES, ids=size_id)
@pytest.mark.parametrize("side", [1, 0], ids=["item-lists", "user-lists"])
def test_list_length_edges(size, side):
    """Lists of every length at and beside the scorer's periods (tile 16, pass 64, chunk 256:
    one chunk, two, three, 9 and 17) and the Gram kernel's (slab 16, slice 2048: one work item,
    a split list of 2 partials, of 3 partials (item side), a zero-length work item, the slab
    buffer carried from one item to the next), each with an uncoupled query from the empty
    partner, one from a short-list partner and a coupled one whose dup row is the list's last.
    K = 3.  The two small sizes compare every query; the others lengths LADDER_SAMPLE, variants
    a and c."""
    model, k = size
    U, I, train, qu, qi, kinds = ladder_problem(side)
    tu, ti, _ = train
    deg = [np.bincount(tu, minlength=U), np.bincount(ti, minlength=I)]
    ent = [qu, qi]
    parts = sorted(-(-int(deg[side][e]) // BIG_SLICE) for e in set(int(e) for e in ent[side]))
    assert parts.count(0) == 1 and parts.count(2) >= 1 and (side == 0 or parts.count(3) == 1), parts
    assert gram_items(deg[side], ent[side]) == (21 if side == 1 else 18)
    p = params_for(size, U, I, 3)
    m = RawModel(model, k, U, I, train, p, prepare=False)
    prepare(m, size, qu, qi)
    res = m.batch(qu, qi, 3)
    tag = "ladder %s k=%d side=%d" % (model, k, side)
    check_lists(res, exact_for(("ladder", side), size, p, train), qu, qi, 3, tag)
    if size in SMALL:
        idx = list(range(qu.size))
    else:
        idx = [q for q, (n, v) in enumerate(kinds) if n in LADDER_SAMPLE and v in "ac"]
        assert len(idx) == 2 * len(LADDER_SAMPLE & set(n for n, _ in kinds)) - 1
    want = oracle_results(("ladder", side), size, p, train, qu[idx], qi[idx])
    assert want[0]["n"] == 0                         # the empty partner on the empty list: x all NaN
    check_against_oracle(take(res, idx), want, 3, tag)
    for q, (n, v) in enumerate(kinds):
        if v == "c":
            assert assert_dup_bits(res, q, tag) == 1
    m.close()


# ---------------------------------------------------------------------------------------
# 2. query-group sizes
# ---------------------------------------------------------------------------------------
GROUPS = (1, 15, 16, 17, 31, 32, 33, 65)
GROUPS_LARGE_K = (17, 33)
GROUP_LIST = 300                         # one full chunk and one of 44 ratings


@functools.lru_cache(maxsize=None)
def group_problem(groups):
    """Item j has a 300-rating list and is queried by groups[j] distinct users with short
    lists, all groups in one batch in shuffled order.  In every group of >= 17 the queries at
    ranks 0, 16 and G - 1 (by batch order) are raters of the item: train pairs, coupled, their
    dup row in either 16-query half of the scoring block.  The others have not rated any of the
    long lists.  Returns U, I, train, qu, qi, coupled (bool per query)."""
    rng = np.random.default_rng(83)
    J, P, NQ, NF = len(groups), 1200, sum(groups), 10
    U, I = P + NQ, J + NF
    raters = [rng.choice(P, GROUP_LIST, replace=False) for _ in range(J)]
    fill = P + np.arange(NQ)
    tu = np.concatenate(raters + [fill, fill]).astype(np.int32)
    ti = np.concatenate([np.full(GROUP_LIST, j) for j in range(J)] +
                        [J + np.arange(NQ) % NF, J + (np.arange(NQ) + 3) % NF]).astype(np.int32)
    perm = rng.permutation(tu.size)
    tu, ti = tu[perm], ti[perm]
    tr = rng.integers(1, 6, tu.size).astype(np.float32)
    assert list(np.bincount(ti, minlength=I)[:J]) == [GROUP_LIST] * J
    assert np.bincount(tu, minlength=U).max() <= 20
    qi = np.repeat(np.arange(J), groups)[rng.permutation(NQ)].astype(np.int32)
    qu = np.zeros(NQ, np.int32)
    coupled = np.zeros(NQ, bool)
    rank = [0] * J
    nxt = 0
    for t in range(NQ):
        j, G = int(qi[t]), groups[int(qi[t])]
        if G >= 17 and rank[j] in (0, 16, G - 1):
            qu[t], coupled[t] = raters[j][rank[j]], True
        else:
            qu[t], nxt = fill[nxt], nxt + 1
        rank[j] += 1
    return U, I, (tu, ti, tr), qu, qi, coupled


@pytest.mark.parametrize("size", SIZES, ids=size_id)
@pytest.mark.parametrize("K", [0, 1])
def test_query_group_sizes(size, K):
    """Entity groups of 1, 15, 16, 17, 31, 32, 33 and 65 queries on two-chunk lists: the
    one-half scoring variant, the two-half variant (17 .. 32 queries: the second half holds 1,
    15 and 16), a second query block of 1 and a third (65 = 32 + 32 + 1), coupled and uncoupled
    queries of one item in one block (records from k_big_solve and from k_bs_back).  Every
    query against the oracle (the three larger sizes: the groups of 17 and 33 only, every
    query); the same queries in another batch order keep every bit."""
    model, k = size
    groups = GROUPS if size in SMALL else GROUPS_LARGE_K
    U, I, train, qu, qi, coupled = group_problem(groups)
    tu, ti, _ = train
    assert list(np.bincount(qi, minlength=I)[:len(groups)]) == list(groups)
    assert coupled.sum() == sum(len({0, 16, G - 1}) for G in groups if G >= 17)   # (G = 17: ranks 0 and 16)
    in_train = np.array([((tu == u) & (ti == i)).sum() for u, i in zip(qu, qi)])
    assert np.array_equal(in_train, coupled.astype(int))
    assert np.unique(qu.astype(np.int64) * I + qi).size == qu.size
    p = params_for(size, U, I, 4)
    m = RawModel(model, k, U, I, train, p, prepare=False)
    prepare(m, size, qu, qi)
    res = m.batch(qu, qi, K)
    tag = "groups %s k=%d K=%d" % (model, k, K)
    want = oracle_results(("groups", groups), size, p, train, qu, qi)
    check_against_oracle(res, want, K, tag)
    for q in np.nonzero(coupled)[0]:
        assert assert_dup_bits(res, q, tag) == 1
    order = np.random.default_rng(84).permutation(qu.size)
    assert (order != np.arange(qu.size)).sum() > qu.size // 2
    again = m.batch(qu[order], qi[order], K)
    for t, q in enumerate(order):
        same_query_bits(again, t, res, q, K, (tag, int(q)))
    m.close()


# ---------------------------------------------------------------------------------------
# 3. more coupled queries than resident workgroups
# ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def coupled_problem(C):
    """C train pairs (c, c) of distinct users and items, each user with 3 or 5 more ratings
    (lists of at most 8), and 40 uncoupled queries (a, a + 3) whose user and item both belong to
    coupled queries too, spread evenly through the batch."""
    U = I = C + 50
    rows = [(c, c) for c in range(C)]
    for c in range(C):
        rows += [(c, (c + d) % I) for d in ((7, 19, 101, 211, 307) if c % 4 == 0 else (7, 19, 101))]
    rows = np.array(rows, np.int32)
    assert np.unique(rows[:, 0].astype(np.int64) * I + rows[:, 1]).size == rows.shape[0]
    rng = np.random.default_rng(97)
    rows = rows[rng.permutation(rows.shape[0])]
    tu, ti = np.ascontiguousarray(rows[:, 0]), np.ascontiguousarray(rows[:, 1])
    tr = rng.integers(1, 6, tu.size).astype(np.float32)
    assert max(np.bincount(tu).max(), np.bincount(ti).max()) <= 40
    qs = [(c, c, True) for c in range(C)]
    for t in range(40):
        a = (13 * t + 5) % (C - 3)
        qs.insert(1 + t * (C // 40) + t, (a, a + 3, False))
    qu = np.array([q[0] for q in qs], np.int32)
    qi = np.array([q[1] for q in qs], np.int32)
    return U, I, (tu, ti, tr), qu, qi, np.array([q[2] for q in qs])


@pytest.mark.parametrize("size", SIZES, ids=size_id)
def test_coupled_persistent(size):
    """2 CUs + 37 coupled queries: k_big_solve's grid is the resident workgroups (one per CU at
    these sizes), so every workgroup walks to a second and a third system, re-using its scratch
    slab and LDS.  Bitwise the same x, influence and top-1 as the same queries in batches of 64
    (every workgroup one system at most), and the oracle on the first and the last query, the
    coupled queries around number CU count, the batch positions around it and 12 random ones
    (the two small sizes: every query)."""
    import torch
    model, k = size
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    C = 2 * cus + 37
    U, I, train, qu, qi, coupled = coupled_problem(C)
    tu, ti, _ = train
    Q = qu.size
    assert coupled.sum() == C and Q == C + 40
    pairs = set(zip(tu.tolist(), ti.tolist()))
    assert all(((int(u), int(i)) in pairs) == bool(c) for u, i, c in zip(qu, qi, coupled))
    p = params_for(size, U, I, 5)
    m = RawModel(model, k, U, I, train, p, prepare=False)
    prepare(m, size, qu, qi)
    res = m.batch(qu, qi, 1)
    tag = "coupled %s k=%d C=%d" % (model, k, C)
    check_lists(res, exact_for(("coupled", C), size, p, train), qu, qi, 1, tag)
    for b0 in range(0, Q, 64):
        part = m.batch(qu[b0:b0 + 64], qi[b0:b0 + 64], 1)
        for t in range(part["offsets"].size - 1):
            same_query_bits(part, t, res, b0 + t, 1, (tag, b0 + t))
    if size in SMALL:
        idx = list(range(Q))
    else:
        cpos = np.nonzero(coupled)[0]
        idx = {0, Q - 1, cus - 1, cus, cus + 1} | set(int(cpos[c]) for c in (0, C - 1, cus - 1, cus, cus + 1))
        idx = sorted(idx | set(int(q) for q in np.random.default_rng(5).choice(Q, 12, replace=False)))
    want = oracle_results(("coupled", C), size, p, train, qu[idx], qi[idx])
    check_against_oracle(take(res, idx), want, 1, tag)
    m.close()


# ---------------------------------------------------------------------------------------
# 4. system counts of the batched panels, 5. a given x, 6b. the merge kernels on short lists
# ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def counts_problem():
    """300 x 40 dense-ish train rows (user lists ~13, item lists ~100) plus: the pair of row
    11 once more with another rating (a pair twice in train), user 300 / item 40 whose only
    ratings are two rows of the pair (300, 40), and user 301 / item 41 without ratings.
    Returns U, I, train, uncoupled (9 pairs), coupled (3 train pairs, the first twice in
    train), tiny (300, 40), empty (301, 41), more (40 further pairs: 16 random ones and 24
    users on item 7, a group whose second 16-query half feeds the merges)."""
    rng, (tu, ti, tr) = dense_problem(91, 300, 40, 4000)
    pairs = set(zip(tu.tolist(), ti.tolist()))
    tu = np.concatenate([tu, [tu[11], 300, 300]]).astype(np.int32)
    ti = np.concatenate([ti, [ti[11], 40, 40]]).astype(np.int32)
    tr = np.concatenate([tr, [float(tr[11]) % 5 + 1, 2.0, 5.0]]).astype(np.float32)
    free = []
    while len(free) < 25:
        pr = (int(rng.integers(0, 300)), int(rng.integers(0, 40)))
        if pr not in pairs and pr not in free:
            free.append(pr)
    shared = [(int(u), 7) for u in rng.permutation(300) if (int(u), 7) not in pairs and (int(u), 7) not in free][:24]
    coupled = [(int(tu[j]), int(ti[j])) for j in (11, 500, 900)]
    assert len(set(coupled)) == 3 and len(shared) == 24
    return 302, 42, (tu, ti, tr), free[:9], coupled, (300, 40), (301, 41), free[9:] + shared


def split(qs):
    return np.array([q[0] for q in qs], np.int32), np.array([q[1] for q in qs], np.int32)


@pytest.mark.parametrize("size", SIZES, ids=size_id)
def test_system_counts(size):
    """Batches of 9, 1, 3 (all coupled: the side list stays empty), 2, 4, 5, 8 and 9 queries on
    one context, one after another: 2, 4, 8, 10, 16 and 18 side systems around the 8-wide
    rounding of the k_bs_trail grid, k_bs_* launches with nothing to do, and a batch with no
    coupled query after one with only coupled queries.  Every query of every batch against the
    oracle; a query that appears in several batches has the same bits in each.  K = 2."""
    model, k = size
    K = 2
    U, I, train, unc, cpl, _, _, _ = counts_problem()
    tu, ti, _ = train
    assert ((tu == cpl[0][0]) & (ti == cpl[0][1])).sum() == 2
    p = params_for(size, U, I, 6)
    m = RawModel(model, k, U, I, train, p)
    seen = {}
    worst_i = worst_x = 0.0
    for qs in (unc, unc[:1], cpl, unc[:2], unc[:4], unc[:5], unc[:8], unc):
        qu, qi = split(qs)
        res = m.batch(qu, qi, K)
        tag = "systems %s k=%d Q=%d%s" % (model, k, len(qs), " coupled" if qs is cpl else "")
        want = oracle_results("counts", size, p, train, qu, qi)
        wi, wx, _ = check_against_oracle(res, want, K, tag)
        worst_i, worst_x = max(worst_i, wi), max(worst_x, wx)
        for t, pr in enumerate(qs):
            if pr in seen:
                same_query_bits(res, t, seen[pr][0], seen[pr][1], K, (tag, pr))
            else:
                seen[pr] = (res, t)
        if qs is cpl:
            assert [assert_dup_bits(res, t, tag) for t in range(3)] == [2, 1, 1]
    print("systems %s k=%d: worst influence %.2e, worst x %.2e over the 8 batches" % (model, k, worst_i, worst_x))
    m.close()


def batch_x(m, qu, qi, x, K):
    """fia_query_batch_x through influence._lib (as RawModel.batch, with the given x [Q, D]); the
    ABI has no x output there: `x` is x_in read back from the device after the call."""
    t = m.torch
    dqu, dqi = m.dev_queries(qu, qi)
    off, tot = m.ctx.count_related(dqu, dqi)
    Q, D = len(qu), m.ctx.num_params()
    xin = t.from_numpy(np.ascontiguousarray(x, np.float64).reshape(-1)).to(m.dev)
    rel = t.full((max(tot, 1),), -7, dtype=t.int32, device=m.dev)
    infl = t.full((max(tot, 1),), float("nan"), dtype=t.float64, device=m.dev)
    tp = t.zeros(max(Q * K, 1), dtype=t.int64, device=m.dev)
    tix = t.zeros(max(Q * K, 1), dtype=t.int64, device=m.dev)
    tv = t.zeros(max(Q * K, 1), dtype=t.float64, device=m.dev)
    m.ctx.query_batch_x(dqu, dqi, off, tot, xin, rel, infl, K, tp, tix, tv)
    t.cuda.synchronize(m.dev)
    return dict(offsets=off.cpu().numpy(), rel_idx=rel[:tot].cpu().numpy().astype(np.int64),
                influence=infl[:tot].cpu().numpy(), x=xin.cpu().numpy().reshape(Q, D),
                topk_pos=tp.cpu().numpy().reshape(Q, K), topk_idx=tix.cpu().numpy().reshape(Q, K),
                topk_val=tv.cpu().numpy().reshape(Q, K))


@pytest.mark.parametrize("size", SIZES, ids=size_id)
def test_query_batch_x(size):
    """fia_query_batch_x (k_big_record_x) on a batch of 9 uncoupled queries, two coupled ones
    (one of a pair twice in train) and one without related ratings.  (i) given the fused call's
    own x: the oracle's influence within RTOL, top-1 by check_topk, x_in left as it was (the
    call has no x output); (ii) given twice that: exactly twice the influence of (i), bitwise
    (every term is linear in x, the factor a power of two); (iii) given a random x: within
    RTOL of (2 e G + wd M theta) x / n from the oracle's G, e, theta; (iv) the fused call
    again: the first fused run's bits."""
    model, k = size
    K = 1
    U, I, train, unc, cpl, _, empty, _ = counts_problem()
    qu, qi = split(unc + cpl[:2] + [empty])
    p = params_for(size, U, I, 6)
    m = RawModel(model, k, U, I, train, p)
    want = oracle_results("counts", size, p, train, qu, qi)
    assert [o["n"] > 0 for o in want] == [True] * 11 + [False]
    tag = "given x %s k=%d" % (model, k)
    first = m.batch(qu, qi, K)
    check_against_oracle(first, want, K, tag + " fused")
    same = batch_x(m, qu, qi, first["x"], K)                                     # (i)
    assert np.array_equal(bits(same["x"]), bits(first["x"]))
    check_against_oracle(same, want, K, tag + " (i)")
    twice = batch_x(m, qu, qi, 2.0 * first["x"], K)                              # (ii)
    assert np.array_equal(twice["rel_idx"], same["rel_idx"])
    assert np.array_equal(bits(twice["influence"]), bits(2.0 * same["influence"]))
    assert np.array_equal(twice["topk_pos"], same["topk_pos"])
    assert np.array_equal(bits(twice["topk_val"]), bits(2.0 * same["topk_val"]))
    D = first["x"].shape[1]                                                      # (iii)
    xr = np.random.default_rng(17).standard_normal((qu.size, D))
    given = batch_x(m, qu, qi, xr, K)
    assert np.array_equal(given["rel_idx"], same["rel_idx"])
    M = np.concatenate([np.ones(2 * k), np.zeros(2)]) if model == "MF" else np.ones(D)
    worst = 0.0
    offs = given["offsets"]
    for q, o in enumerate(want):
        b, e = offs[q], offs[q + 1]
        assert e - b == o["n"]
        if o["n"]:
            ref = (2.0 * o["e"][:, None] * o["G"] + (WD * M * o["theta"])[None, :]) @ xr[q] / o["n"]
            err = rel_err(given["influence"][b:e], ref)
            assert err < RTOL, (tag, q, err)
            worst = max(worst, err)
            pos = given["topk_pos"][q]
            check_topk(pos, given["influence"][b:e], ref, K)
            assert given["topk_idx"][q][0] == given["rel_idx"][b:e][pos[0]]
            assert bits(given["topk_val"][q])[0] == bits(given["influence"][b:e])[pos[0]]
        else:
            assert given["topk_pos"][q][0] == -1 and np.isnan(given["topk_val"][q][0])
    print("%s (iii): 12 queries with a random x vs the oracle's gradients, worst influence %.2e" % (tag, worst))
    for q in (9, 10):
        assert_dup_bits(given, q, tag)
    again = m.batch(qu, qi, K)                                                   # (iv)
    for q in range(qu.size):
        same_query_bits(again, q, first, q, K, (tag, q))
    m.close()


# ---------------------------------------------------------------------------------------
# 6. the top-K merge kernels behind this path's candidates
# ---------------------------------------------------------------------------------------
def merge_kernel(Q, total, K):
    """launch_topk_merge's rule: row (K = 1), thread (K <= 4) while the batch has at most 16
    candidate chunks per query on average, else a wave per query."""
    few = 2 * Q + total // RUN_CHUNK + 1 <= 16 * Q
    return "row" if few and K == 1 else "thread" if few and K <= 4 else "wave"


def merges_long_list(size):
    """(a) The wave merge (k_topk_merge) over 17 item-side chunks x 4 passes of candidates: the
    coupled query on the 4097-list and a query whose whole related list has fewer than 64
    entries in one batch, K = 1, 4 and 64 (the short query: -1 / NaN padding)."""
    model, k = size
    U, I, train, lqu, lqi, kinds = ladder_problem(1)
    sel = [kinds.index((4097, "c")), kinds.index((15, "b"))]
    qu, qi = lqu[sel], lqi[sel]
    p = params_for(size, U, I, 3)
    m = RawModel(model, k, U, I, train, p, prepare=False)
    prepare(m, size, qu, qi)
    want = oracle_results(("ladder", 1), size, p, train, qu, qi)
    assert want[0]["n"] > 4097 and 0 < want[1]["n"] < 64
    for K in (1, 4, 64):
        res = m.batch(qu, qi, K)
        assert merge_kernel(2, int(res["offsets"][-1]), K) == "wave"
        check_against_oracle(res, want, K, "merge long %s k=%d K=%d" % (model, k, K))
        assert (res["topk_pos"][1][want[1]["n"]:] == -1).all()
    m.close()


def merges_short_lists(size, tmp_path):
    """(b) 40 queries with lists of ~110 entries, 24 of them on one item (the candidates of the
    scorer's second 16-query half, K > 1 included), a pair twice in train and the pair (300, 40)
    whose two train rows are its whole related list [a, b, a, b], through the facade with
    K = 1, 4, 5: the row, the thread and the wave merge.  The copies of a row tie bit for bit
    and the lower position comes first."""
    model, k = size
    U, I, train, _, cpl, tiny, _, more = counts_problem()
    qu, qi = split(more + [cpl[0], tiny])
    assert np.bincount(qi).max() >= 24
    tq = qu.size - 1
    p = params_for(size, U, I, 6)
    m = make_model(model, U, I, k, train, (qu, qi), p, tmpdir=tmp_path)
    want = oracle_results("counts", size, p, train, qu, qi)
    assert want[tq]["n"] == 4 and np.array_equal(want[tq]["rel"][:2], want[tq]["rel"][2:])
    for K, kernel in ((1, "row"), (4, "thread"), (5, "wave")):
        res = m.get_influence_batch(list(range(qu.size)), K=K)
        assert merge_kernel(qu.size, int(res["offsets"][-1]), K) == kernel
        tag = "merge short %s k=%d K=%d" % (model, k, K)
        check_against_oracle(res, want, K, tag)
        assert assert_dup_bits(res, tq - 1, tag) == 2 and assert_dup_bits(res, tq, tag) == 2
        pos = res["topk_pos"][tq]
        assert pos[0] in (0, 1)                      # of the two tied copies the lower position
        if K >= 4:
            assert list(pos[:4]) == [pos[0], pos[0] + 2, 1 - pos[0], 3 - pos[0]] and (pos[4:] == -1).all()
    m.ctx.close()


@pytest.mark.parametrize("size", SIZES, ids=size_id)
def test_topk_merges(size, tmp_path):
    """The three merge kernels (launch_topk_merge) on this path's four candidates per chunk and
    query: see merges_long_list and merges_short_lists; which kernel a batch takes is
    established from its Q, total and K by the launcher's rule."""
    merges_long_list(size)
    merges_short_lists(size, tmp_path)


# ---------------------------------------------------------------------------------------
# 7. fia_prepare_for of a few entities at k = 256
# ---------------------------------------------------------------------------------------
PREPARE_SETS = [((17,), "a"), ((4097, 2049, 1, 65), "ac"), ((4097, 2049, 1, 65, 257), "ac"),
                ((4097, 2049, 1, 65, 257, 513), "ac")]


@pytest.mark.parametrize("size", [("MF", 256), ("NCF", 256), ("NCF", 128)], ids=size_id)
def test_prepare_for_small_sets(size):
    """fia_prepare_for of query sets that make 1, 7, 8 and 9 item-side Gram work items (the
    4097-list is 3 of them, the 2049-list 2: split lists and their combine in a compacted
    cache) on the ladder problem.  NCF k = 256 is the size with the XCD-ordered 1-D Gram grid,
    whose padding to 8 work items matters exactly at such counts.  Every query of a set against
    the oracle; a query outside the set is refused until the next prepare; after fia_prepare_for
    of the union of the sets every query has the same bits as before.  K = 3."""
    from influence._lib import FIAError
    model, k = size
    K = 3
    U, I, train, lqu, lqi, kinds = ladder_problem(1)
    tu, ti, _ = train
    deg_u, deg_i = np.bincount(tu, minlength=U), np.bincount(ti, minlength=I)
    p = params_for(size, U, I, 3)
    m = RawModel(model, k, U, I, train, p, prepare=False)
    outside = kinds.index((15, "b"))
    runs = []
    for (lengths, variants), n_items in zip(PREPARE_SETS, (1, 7, 8, 9)):
        sel = [q for q, (n, v) in enumerate(kinds) if n in lengths and v in variants]
        assert len(sel) == len(lengths) * len(variants)
        qu, qi = lqu[sel], lqi[sel]
        assert gram_items(deg_i, qi) == n_items and gram_items(deg_u, qu) == len(set(qu.tolist()))
        assert lqu[outside] not in qu and lqi[outside] not in qi
        m.prepare_for(qu, qi)
        res = m.batch(qu, qi, K)
        want = oracle_results(("ladder", 1), size, p, train, qu, qi)
        check_against_oracle(res, want, K, "prepare_for %s k=%d, %d Gram items" % (model, k, n_items))
        with pytest.raises(FIAError):
            m.batch(lqu[outside:outside + 1], lqi[outside:outside + 1], K)
        runs.append((sel, res))
    union = sorted(set(q for sel, _ in runs for q in sel))
    m.prepare_for(lqu[union], lqi[union])
    full = m.batch(lqu[union], lqi[union], K)
    for sel, res in runs:
        for t, q in enumerate(sel):
            same_query_bits(res, t, full, union.index(q), K, (model, k, q))
    m.close()
