"""The problems of test_gpu_grouped_score.py (the entity-shared VALU scorers k_score_grouped_mf
and k_score_ncf, the group builder and the solves and Gram kernels behind them) and, in pure
numpy, the facts those tests claim about them: how many work items, scoring trips, scan tiles
and merge kernel a batch means, the sizes of its query groups, and where in a list the test
pair's own train row sits.  Nothing here touches the GPU: test_grouped_problems_cpu.py runs the
same claims, and a sample of every problem through the oracle, where there is none.

The schedule restated from the input alone:
  work items   n_items = sum over entities with a non-empty query group of
               ceil(deg / 256) * ceil(group / QB),  QB = 8 (MF k = 32, NCF k = 32), 16 (MF k = 64)
  scoring grid min(ceil(max_chunks / 4), cap) workgroups of 4 waves, a wave per work item,
               max_chunks = 2 Q + total_rel / 128 + 1, cap = 8192 (MF), 1024 (NCF)
  group scan   U + I + 1 words (the total last) in tiles of 512, look-back windows of 64 tiles
  top-K merge  K = 1: a 16-lane row per query, K <= 4: a thread per query, both while
               max_chunks <= 16 Q; otherwise a wave per query
All problems: wd = 1e-3, damping = 1e-6, parameters from synth.mf_params / synth.ncf_params."""
import functools

import numpy as np

from influence import synth
from test_gpu_mfma_score import dense_problem
from test_gpu_parity import NEAR_TIE     # check_topk's swap tolerance

WD, DAMPING = 1e-3, 1e-6
SIZES = [("MF", 32), ("MF", 64), ("NCF", 32)]
KS = {"MF": (2, 4, 5, 64), "NCF": (0, 1, 2, 4, 5, 64)}      # K <= 1 at MF is the MFMA kernel
QB = {("MF", 32): 8, ("MF", 64): 16, ("NCF", 32): 8}        # query_block<M>()
CHUNK = 256                              # kChunk
MERGE_CLEN = 128                         # kRunChunk: the chunk length max_chunks is counted in
GRID_CAP = {"MF": 8192, "NCF": 1024}
WAVES = 4                                # work items per workgroup and trip
SCAN_TILE = 512                          # kScanTile
SOLVE_TILE_CAP = 2048                    # k_solve_tile: persistent beyond 8 * 256 CUs queries
COUPLED_CAP = 256                        # k_solve at k >= 32: persistent beyond 256 coupled queries


def size_id(v):
    return "%s-%d" % v if isinstance(v, tuple) else None


def params_for(model, U, I, k, seed):
    return synth.mf_params(U, I, k, seed) if model == "MF" else synth.ncf_params(U, I, k, seed)


# ---------------------------------------------------------------------------------------
# the schedule, from (train, queries) alone
# ---------------------------------------------------------------------------------------
def degrees(train, U, I):
    tu, ti, _ = train
    return np.bincount(tu, minlength=U), np.bincount(ti, minlength=I)


def total_related(train, U, I, qu, qi):
    deg_u, deg_i = degrees(train, U, I)
    return int((deg_u[qu] + deg_i[qi]).sum())


def group_sizes(train, U, I, qu, qi):
    """Queries per user and per item, over the queries k_group_count ranks (n_q > 0)."""
    deg_u, deg_i = degrees(train, U, I)
    ok = deg_u[qu] + deg_i[qi] > 0
    return np.bincount(qu[ok], minlength=U), np.bincount(qi[ok], minlength=I)


def work_items(train, U, I, qu, qi, qb):
    """n_items = wstart[U + I] of k_group_scan."""
    n = 0
    for deg, grp in zip(degrees(train, U, I), group_sizes(train, U, I, qu, qi)):
        n += int((((deg + CHUNK - 1) // CHUNK) * ((grp + qb - 1) // qb))[grp > 0].sum())
    return n


def max_chunks(Q, total):
    return 2 * Q + total // MERGE_CLEN + 1


def score_trips(model, n_items, Q, total):
    """Trips of the busiest wave's grid-stride loop."""
    grid = min(max((max_chunks(Q, total) + WAVES - 1) // WAVES, 1), GRID_CAP[model])
    return (n_items + WAVES * grid - 1) // (WAVES * grid)


def merge_kernel(Q, total, K):
    small = max_chunks(Q, total) <= 16 * Q
    if K == 1 and small and Q <= 16384:
        return "row"
    return "thread" if K <= 4 and small else "wave"


def scan_tiles(U, I):
    return (U + I + 1 + SCAN_TILE - 1) // SCAN_TILE


class Lists(object):
    """Both sides' lists in index order (train rows stably sorted by entity, as the oracle's
    CsrExact and the related lists have them)."""

    def __init__(self, train, U, I):
        self.tu, self.ti, _ = train
        self.I = I
        self.side = []
        for ids, n in ((self.tu, U), (self.ti, I)):
            order = np.argsort(ids, kind="stable")
            self.side.append((order, np.searchsorted(ids[order], np.arange(n + 1), side="left")))

    def rows(self, sd, e):
        order, ptr = self.side[sd]
        return order[ptr[e]:ptr[e + 1]]

    def dup_positions(self, u, i):
        """List positions of the rows of the pair (u, i): in R_u, in C_i (the entries of a
        query (u, i) that take the kernels' dup branch)."""
        return (np.nonzero(self.ti[self.rows(0, u)] == i)[0], np.nonzero(self.tu[self.rows(1, i)] == u)[0])

    def in_train(self, qu, qi):
        return np.isin(np.asarray(qu, np.int64) * self.I + qi, self.tu.astype(np.int64) * self.I + self.ti)


# ---------------------------------------------------------------------------------------
# the oracle, once per problem
# ---------------------------------------------------------------------------------------
_ORACLE_CACHE = {}


def oracle_results(key, model, k, p, train, qu, qi):
    """CsrExact results (rel, n, influence, x) of every query, computed once per problem and
    shared (read-only); a pair that occurs twice in a batch is solved once.  A train row that
    is in the related list twice (the test pair's own row: once per side) has one influence,
    but the oracle's two copies of it differ by an ulp or so; both get the first copy's value,
    so that the oracle ranks them by position, as the build's tie rule says."""
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
                _, first, inv = np.unique(o["rel"], return_index=True, return_inverse=True)
                memo[pair]["influence"] = o["influence"][first[inv]]
            out.append(memo[pair])
        _ORACLE_CACHE[key] = out
    return _ORACLE_CACHE[key]


def assert_no_near_ties(want, K=64):
    """On the oracle's values: no query has two distinct train rows within NEAR_TIE * max among
    its K + 1 largest |influence| -- check_topk's tolerance then has nothing to forgive, and the
    tests assert 0 swaps.  (The copies of the test pair's own row are equal: oracle_results.)"""
    for q, o in enumerate(want):
        if o["n"] < 2:
            continue
        a = np.abs(o["influence"])
        first = np.lexsort((np.arange(a.size), -a))[:K + 1]
        v, rows = a[first], o["rel"][first]
        for t in np.nonzero(v[:-1] - v[1:] <= NEAR_TIE * v[0])[0]:
            assert rows[t] == rows[t + 1] and v[t] == v[t + 1], (q, int(first[t]), int(first[t + 1]), v[t], v[t + 1])


# ---------------------------------------------------------------------------------------
# 1. list-length edges
# ---------------------------------------------------------------------------------------
LENGTHS = [1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 511, 512, 513, 769]
DUP_LISTS = (257, 513)                   # also queried by the raters at DUP_AT
DUP_AT = (63, 64, 127, 128, 191, 192, 255, 256)     # every lane row's first and last entry, chunk 1's first
TWICE_AT = (5, 256)                      # the 257-list: one rater holds both positions
EDGE_SEED = 71


@functools.lru_cache(maxsize=None)
def edge_problem(side):
    """One long-list entity per length in LENGTHS plus one without ratings (side 1: items hold
    the lists; side 0: the transposed problem, users hold them), the train rows permuted so
    that list order is train-row order and not id order.  The 257-list's last entry (chunk 1)
    is a second row of the rater at position 5, with another rating.  Per list: the raters at
    the first and the last position, on the 257- and 513-lists also those at DUP_AT, a non-rater
    with a non-empty list and the entity with no ratings; one pair on the unrated list; one
    query with n_q = 0 in the middle of the batch.
    Returns U, I, train, qu, qi, dups [(query, list length, list position of its own train
    row)], the index of the empty query."""
    rng = np.random.default_rng(EDGE_SEED)
    U, I = 900, len(LENGTHS) + 1
    raters = [rng.choice(U - 1, n, replace=False).astype(np.int32) for n in LENGTHS]
    tu = np.concatenate(raters)
    ti = np.concatenate([np.full(r.size, j, np.int32) for j, r in enumerate(raters)])
    N = tu.size
    perm = rng.permutation(N)
    tu, ti = tu[perm], ti[perm]
    tr = rng.integers(1, 6, N).astype(np.float32)
    rows = np.nonzero(ti == LENGTHS.index(257))[0]
    tu[rows[TWICE_AT[1]]] = tu[rows[TWICE_AT[0]]]
    tr[rows[TWICE_AT[1]]] = tr[rows[TWICE_AT[0]]] % 5 + 1
    deg_u = np.bincount(tu, minlength=U)
    qs = []                                        # (user, item, list length, position of the pair's row or -1)
    for j, n in enumerate(LENGTHS):
        order = tu[ti == j]                        # item j's list in index (train-row) order
        at = sorted({0, n - 1} | (set(DUP_AT) if n in DUP_LISTS else set()))
        qs += [(int(order[pos]), j, n, pos) for pos in at]
        others = np.setdiff1d(np.nonzero(deg_u > 0)[0], order)
        qs += [(int(rng.choice(others)), j, n, -1), (U - 1, j, n, -1)]
    qs.append((int(raters[5][0]), I - 1, 0, -1))
    if side == 0:
        U, I, tu, ti = I, U, ti, tu
        qs = [(i, u, n, pos) for u, i, n, pos in qs]
    mid = len(qs) // 2
    qs.insert(mid, (U - 1, I - 1, 0, -1))
    qu = np.array([q[0] for q in qs], np.int32)
    qi = np.array([q[1] for q in qs], np.int32)
    dups = [(t, q[2], q[3]) for t, q in enumerate(qs) if q[3] >= 0]
    return U, I, (tu, ti, tr), qu, qi, dups, mid


def assert_edge_claims(side):
    """The list lengths, the dup positions (from the index order), the twice-held pair, the
    empty query; returns the problem."""
    U, I, train, qu, qi, dups, empty = edge_problem(side)
    tu, ti, tr = train
    deg = degrees(train, U, I)
    assert sorted(deg[side][deg[side] > 0]) == LENGTHS and deg[side][-1] == 0 and deg[1 - side][-1] == 0
    L = Lists(train, U, I)
    seen = set()
    for q, n, pos in dups:
        at = L.dup_positions(int(qu[q]), int(qi[q]))[side]
        assert deg[side][(qu, qi)[side][q]] == n and pos in at, (q, n, pos, at)
        seen.add((n, pos))
    for n in LENGTHS:
        assert (n, 0) in seen and (n, n - 1) in seen, n
    for n in DUP_LISTS:
        for pos in DUP_AT:
            assert (n, pos) in seen, (n, pos)
    twice = [q for q, n, pos in dups if n == 257 and pos == TWICE_AT[1]]
    assert len(twice) == 1
    q2 = twice[0]
    at = L.dup_positions(int(qu[q2]), int(qi[q2]))
    assert list(at[side]) == list(TWICE_AT) and at[1 - side].size == 2
    both = np.nonzero((tu == qu[q2]) & (ti == qi[q2]))[0]
    assert both.size == 2 and tr[both[0]] != tr[both[1]]
    assert 0 < empty < qu.size - 1 and deg[0][qu[empty]] + deg[1][qi[empty]] == 0
    in_train = L.in_train(qu, qi)
    assert in_train.sum() == len(dups) and not in_train[empty]
    # per list a non-rater with a list of its own and the entity without ratings
    other = (qi, qu)[side]
    for e in np.nonzero(deg[side] > 0)[0]:
        mine = ~in_train & ((qu, qi)[side] == e)
        assert (deg[1 - side][other[mine]] > 0).any() and (deg[1 - side][other[mine]] == 0).any(), e
    return U, I, train, qu, qi, dups, empty, q2


# ---------------------------------------------------------------------------------------
# 2. query-group sizes
# ---------------------------------------------------------------------------------------
GROUPS = [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 33]
GROUP_SEED = 72
N_USER0 = 19                             # items user 0 is queried on; one of the queries twice


@functools.lru_cache(maxsize=None)
def group_problem():
    """Item j < 12 has about 300 ratings (two chunks) and item 12 + j at most 64 (one lane row:
    the NCF one-row path); both are queried by GROUPS[j] distinct users, about half of them
    raters of the item (the dup branch in either chunk, for one column of a block).  User 0 is
    in 20 queries on 19 further short-list items, one of them twice (a user-side group of
    several blocks; the repeated query).  Batch order shuffled; a second shuffle of the same
    queries.  Returns U, I, train, qu, qi, order2 (batch 2 is qu[order2], qi[order2])."""
    rng = np.random.default_rng(GROUP_SEED)
    G = len(GROUPS)
    U, I = 600, 2 * G + N_USER0
    us, its = [], []
    for j in range(I):
        n = 290 + 3 * j if j < G else 40 + 2 * (j - G) if j < 2 * G else 6 + j % 5
        us.append(rng.choice(U, n, replace=False))
        its.append(np.full(n, j))
    tu = np.concatenate(us).astype(np.int32)
    ti = np.concatenate(its).astype(np.int32)
    perm = rng.permutation(tu.size)
    tu, ti = tu[perm], ti[perm]
    tr = rng.integers(1, 6, tu.size).astype(np.float32)
    qs = []
    for j in range(2 * G):
        qs += [(int(u), j) for u in rng.choice(np.arange(1, U), GROUPS[j % G], replace=False)]
    qs += [(0, j) for j in range(2 * G, I)]
    qs.append(qs[-3])                              # the repeated query
    order = rng.permutation(len(qs))
    qu = np.array([qs[t][0] for t in order], np.int32)
    qi = np.array([qs[t][1] for t in order], np.int32)
    return U, I, (tu, ti, tr), qu, qi, rng.permutation(len(qs))


def assert_group_claims():
    U, I, train, qu, qi, order2 = group_problem()
    G = len(GROUPS)
    deg_u, deg_i = degrees(train, U, I)
    assert ((deg_i[:G] > CHUNK) & (deg_i[:G] <= 2 * CHUNK)).all() and (deg_i[G:] <= 64).all() and (deg_u <= 64).all()
    gu, gi = group_sizes(train, U, I, qu, qi)
    assert list(gi[:G]) == GROUPS and list(gi[G:2 * G]) == GROUPS and gu[0] == N_USER0 + 1
    assert sorted(gi[2 * G:]) == [1] * (N_USER0 - 1) + [2]
    pairs = qu.astype(np.int64) * I + qi
    assert np.unique(pairs).size == pairs.size - 1
    assert not np.array_equal(order2, np.arange(qu.size)) and (np.diff(qi) != 0).any()
    # dup queries on the two-chunk lists: in chunk 0 and in chunk 1, at every lane row
    L = Lists(train, U, I)
    lane_rows = set()
    for q in np.nonzero(L.in_train(qu, qi) & (qi < G))[0]:
        lane_rows.update(int(p) // 64 for p in L.dup_positions(int(qu[q]), int(qi[q]))[1])
    assert lane_rows >= set(range(5)), lane_rows
    return U, I, train, qu, qi, order2


# ---------------------------------------------------------------------------------------
# 3. the second trip of the grid-stride loops
# ---------------------------------------------------------------------------------------
TRIP_Q = {("MF", 32): 16400, ("MF", 64): 16400, ("NCF", 32): 2060}
TRIP_PAIRS = 300                         # queries whose pair is a train row
TRIP_SEED = 73


@functools.lru_cache(maxsize=None)
def trip_problem(Q):
    """Q queries on pairwise distinct users and items, U = I = Q; user u rated items
    P[u], P[u + 1], P[u + 2] (and P[u + 3] if 3 | u) of a random cycle P: three or four ratings
    per user and per item, so each side of a query is one chunk and one block and the batch is
    2 Q work items.  TRIP_PAIRS of the queries are train pairs (u, P[u]); the others go to
    P[u + d], d >= 5 along the cycle of the remaining users.  Train rows and the batch shuffled."""
    rng = np.random.default_rng(TRIP_SEED + Q)
    P = rng.permutation(Q)
    u = np.arange(Q)
    tu = np.concatenate([u, u, u, u[::3]])
    ti = np.concatenate([P[u], P[(u + 1) % Q], P[(u + 2) % Q], P[(u[::3] + 3) % Q]])
    perm = rng.permutation(tu.size)
    tu, ti = tu[perm].astype(np.int32), ti[perm].astype(np.int32)
    tr = rng.integers(1, 6, tu.size).astype(np.float32)
    pair = np.zeros(Q, bool)
    pair[rng.choice(Q, TRIP_PAIRS, replace=False)] = True
    rest = np.nonzero(~pair)[0]
    to = u.copy()
    to[rest] = np.roll(rest, -5)
    qu = rng.permutation(Q).astype(np.int32)
    qi = P[to[qu]].astype(np.int32)
    return Q, Q, (tu, ti, tr), qu, qi


def assert_trip_claims(model, k):
    Q = TRIP_Q[(model, k)]
    U, I, train, qu, qi = trip_problem(Q)
    assert np.unique(qu).size == Q and np.unique(qi).size == Q
    deg_u, deg_i = degrees(train, U, I)
    assert set(deg_u) == {3, 4} and set(deg_i) == {3, 4}
    total = total_related(train, U, I, qu, qi)
    n_items = work_items(train, U, I, qu, qi, QB[(model, k)])
    assert n_items == 2 * Q > WAVES * GRID_CAP[model] and score_trips(model, n_items, Q, total) == 2
    assert Q > SOLVE_TILE_CAP
    coupled = int(Lists(train, U, I).in_train(qu, qi).sum())
    assert coupled >= TRIP_PAIRS > COUPLED_CAP
    if model == "MF":
        assert scan_tiles(U, I) > 64
    halves = np.array_split(np.arange(Q), 2)
    for part in halves:
        t = total_related(train, U, I, qu[part], qi[part])
        assert score_trips(model, work_items(train, U, I, qu[part], qi[part], QB[(model, k)]), part.size, t) == 1
    return U, I, train, qu, qi, halves


# ---------------------------------------------------------------------------------------
# 4. group-scan tile edges
# ---------------------------------------------------------------------------------------
TILE_NE = (511, 512, 513)                # U + I: the total's word is the tile's last, a tile of its own, second of two


@functools.lru_cache(maxsize=None)
def tile_problem(nE):
    U, I, N = 400, nE - 400, 1500
    rng, (tu, ti, tr) = dense_problem(74, U, I, N)
    qu = rng.integers(0, U, 40).astype(np.int32)
    qi = rng.integers(0, I, 40).astype(np.int32)
    qu[7], qi[19], qu[33], qi[33] = U - 1, I - 1, U - 1, I - 1
    return U, I, (tu, ti, tr), qu, qi


def assert_tile_claims(nE):
    U, I, train, qu, qi = tile_problem(nE)
    assert U + I == nE and scan_tiles(U, I) == (1 if nE < 512 else 2)
    deg_u, deg_i = degrees(train, U, I)
    assert deg_u[U - 1] > 0 and deg_i[I - 1] > 0
    gu, gi = group_sizes(train, U, I, qu, qi)
    assert gu[U - 1] >= 2 and gi[I - 1] >= 2
    return U, I, train, qu, qi


# ---------------------------------------------------------------------------------------
# 5. long lists and Gram slices
# ---------------------------------------------------------------------------------------
LONG = (2100,)                           # 9 chunks
LONG_MF64 = (2100, 4095, 4096, 4097, 8193)     # k = 64 Gram slices of 4,096 rows: one, one, two, three
LONG_SEED = 75


@functools.lru_cache(maxsize=None)
def long_problem(lengths, merge):
    """The last len(lengths) items have that many raters; 29 items share 3,000 further ratings.
    Per long list: a rater, a non-rater with ratings and the user without ratings.  merge =
    "thread": short-list queries are added until max_chunks <= 16 Q."""
    rng = np.random.default_rng(LONG_SEED)
    nl = len(lengths)
    U, I, N = max(lengths) + 800, 29 + nl, 3000
    key = np.sort(rng.choice((U - 1) * 29, N, replace=False))
    us, its = [key // 29], [key % 29]
    for j, n in enumerate(lengths):
        us.append(rng.choice(U - 1, n, replace=False))
        its.append(np.full(n, 29 + j))
    tu = np.concatenate(us).astype(np.int32)
    ti = np.concatenate(its).astype(np.int32)
    perm = rng.permutation(tu.size)
    tu, ti = tu[perm], ti[perm]
    tr = rng.integers(1, 6, tu.size).astype(np.float32)
    deg_u = np.bincount(tu, minlength=U)
    qs = []
    for j in range(nl):
        lst = tu[ti == 29 + j]
        non = np.setdiff1d(np.nonzero(deg_u > 0)[0], lst)
        qs += [(int(lst[len(lst) // 2]), 29 + j), (int(rng.choice(non)), 29 + j), (U - 1, 29 + j)]
    n_short = 0 if merge == "wave" else 12 * nl * nl
    qs += [(int(u), int(i)) for u, i in zip(rng.integers(0, U - 1, n_short), rng.integers(0, 10, n_short))]
    qu = np.array([q[0] for q in qs], np.int32)
    qi = np.array([q[1] for q in qs], np.int32)
    return U, I, (tu, ti, tr), qu, qi


def assert_long_claims(model, k, merge):
    lengths = LONG_MF64 if (model, k) == ("MF", 64) else LONG
    U, I, train, qu, qi = long_problem(lengths, merge)
    deg_u, deg_i = degrees(train, U, I)
    assert tuple(deg_i[29:]) == lengths and deg_u[U - 1] == 0
    Q, total = qu.size, total_related(train, U, I, qu, qi)
    for K in KS[model]:
        want = "wave" if merge == "wave" or K > 4 else "row" if K == 1 else "thread"
        assert merge_kernel(Q, total, K) == want, (K, Q, total)
    L = Lists(train, U, I)
    in_train = L.in_train(qu[:3 * len(lengths)], qi[:3 * len(lengths)])
    assert list(in_train) == [True, False, False] * len(lengths)
    for j, n in enumerate(lengths):                 # the rater's row is in a chunk beyond the first
        assert L.dup_positions(int(qu[3 * j]), int(qi[3 * j]))[1][0] == n // 2 >= CHUNK
        assert deg_u[qu[3 * j + 1]] > 0 and deg_u[qu[3 * j + 2]] == 0
    return U, I, train, qu, qi, lengths


# ---------------------------------------------------------------------------------------
# 7. the first prepare is fia_prepare_for (NCF k = 32)
# ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def subset_problem():
    """12 queries on item 3 (a group of two blocks), a train pair, five more on item 7; a user
    and an item outside the subset."""
    U, I, N = 400, 12, 2500
    rng, (tu, ti, tr) = dense_problem(76, U, I, N)
    users = rng.choice(U, 17, replace=False)
    qs = [(int(u), 3) for u in users[:12]] + [(int(tu[17]), int(ti[17]))] + [(int(u), 7) for u in users[12:]]
    qu = np.array([q[0] for q in qs], np.int32)
    qi = np.array([q[1] for q in qs], np.int32)
    out_u = int(np.setdiff1d(np.arange(U), qu)[0])
    out_i = int(np.setdiff1d(np.arange(I), qi)[0])
    return U, I, (tu, ti, tr), qu, qi, out_u, out_i


def assert_subset_claims():
    U, I, train, qu, qi, out_u, out_i = subset_problem()
    gu, gi = group_sizes(train, U, I, qu, qi)
    assert gi.max() > QB[("NCF", 32)] and Lists(train, U, I).in_train(qu, qi).sum() >= 1
    assert out_u not in qu and out_i not in qi
    return U, I, train, qu, qi, out_u, out_i
