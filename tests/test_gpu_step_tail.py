"""Oracle tests of the tail of the MF k = 16 step: the coupled queries (test pair = a train row)
solved by a role of the fused scan + side-solve launch, with no list and no launch of their own,
and the K = 1 merge of the per-chunk top-1 candidates on a 16-lane row per query.

Every comparison is against the fp64 oracle (oracle.fia_oracle) through the helpers of the
existing suites, at their tolerances: related sets bit-exact, influence and x < RTOL, top-K
exact on the kernel's own values and against the oracle under check_topk's near-tie rule.  The
coupled-role tests use the 600 x 40 problem of test_gpu_scan_solve; the merge tests one problem
of their own (below).  Oracle answers are computed once per pair and shared read-only."""
import numpy as np
import pytest

from influence import synth
from test_gpu_mfma_score import RawModel, WD, DAMPING, check_against_oracle
from test_gpu_parity import RTOL, rel_err
from test_gpu_scan_solve import U, I, model, oracle_for, problem, run, same_bits

pytestmark = pytest.mark.gpu

K16 = 16


# ---------------------------------------------------------------------------------------
# 1. the coupled role
# ---------------------------------------------------------------------------------------
def pairs_of(n_free, seed):
    P = problem()
    rng = np.random.default_rng(seed)
    free = [P["free"][j] for j in rng.choice(len(P["free"]), n_free, replace=False)]
    cpl = [P["train_pairs"][j] for j in rng.choice(len(P["train_pairs"]), 80, replace=False)]
    return free, cpl


def arrays(pairs):
    """The batch in the order given (the role's compaction must not depend on item order)."""
    return np.array([q[0] for q in pairs], np.int32), np.array([q[1] for q in pairs], np.int32)


def coupled_batch(case):
    free, cpl = pairs_of(80, 4242)
    if case == "one-query":
        pairs = cpl[:1]
    elif case == "edges-of-65":
        # the first query, the last of the first solve workgroup, the first of the second = the last
        pairs = free[:65]
        for j, at in enumerate((0, 63, 64)):
            pairs[at] = cpl[j]
    elif case == "all-70":
        pairs = cpl[:70]
    elif case == "none":
        pairs = free[:70]
    else:
        # a coupled query beside queries on its user with an item nobody rated and on its item
        # with a user who rated nothing, and the pair of those two (n = 0)
        cu, ci = cpl[0]
        pairs = free[:20] + [(cu, I - 1), (cu, ci), (U - 1, ci), (U - 1, I - 1)] + free[20:40]
    return arrays(pairs)


@pytest.mark.parametrize("case", ["one-query", "edges-of-65", "all-70", "none", "empty-lists-beside"])
def test_coupled_role(case):
    """Every query of the batch against the oracle, the coupled ones included (x, influence,
    top-1); then the same batch again on the same context: the same bits."""
    qu, qi = coupled_batch(case)
    have = set(problem()["train_pairs"])
    n_cpl = sum((int(u), int(i)) in have for u, i in zip(qu, qi))
    assert n_cpl == {"one-query": 1, "edges-of-65": 3, "all-70": 70, "none": 0, "empty-lists-beside": 1}[case]
    if case == "edges-of-65":
        assert qu.size == 65 and all((int(qu[j]), int(qi[j])) in have for j in (0, 63, 64))
    want = oracle_for(qu, qi)
    m = model()
    first = run(m, qu, qi, K=1)
    check_against_oracle(first, want, 1, "coupled role %s" % case)
    again = run(m, qu, qi, K=1)
    same_bits(first, again)
    m.close()


def test_fused_then_given_x_then_fused():
    """A fused call with coupled queries, fia_query_batch_x on the same context (the scan as a
    launch of its own, no solve role), and the fused call again: the given-x influence is the
    oracle's, and the two fused calls agree bit for bit."""
    qu, qi = coupled_batch("all-70")
    want = oracle_for(qu, qi)
    m = model()
    first = run(m, qu, qi, K=1)
    check_against_oracle(first, want, 1, "fused before given-x")
    x_in = m.torch.from_numpy(np.ascontiguousarray(first["x"].reshape(-1))).to(m.dev)
    given = run(m, qu, qi, K=1, x_in=x_in)
    for q, o in enumerate(want):
        b, e = given["offsets"][q], given["offsets"][q + 1]
        assert np.array_equal(given["rel_idx"][b:e], o["rel"]), q
        assert rel_err(given["influence"][b:e], o["influence"]) < RTOL, q
    qu2, qi2 = coupled_batch("none")
    check_against_oracle(run(m, qu2, qi2, K=1), oracle_for(qu2, qi2), 1, "fused, none coupled, after given-x")
    again = run(m, qu, qi, K=1)
    same_bits(first, again)
    m.close()


# ---------------------------------------------------------------------------------------
# 2. the K = 1 merge on a 16-lane row
# ---------------------------------------------------------------------------------------
# A query has one candidate slot per 128-rating chunk of its user list and of its item list.
# Users (ratings, slots): LONG 4200 (33), B16 2048 (16), C17 2049 (17), ONE 1 (1), TIE 130 rows
# that are all (TIE, JT, 3.0) (2 slots of equal candidates), NOBODY 0.  Items: J0 rated by 40
# small users (1 slot), JT by TIE's 130 rows alone (2 slots of equal candidates), NOTHING by none.
MU, MI = 60, 4300
LONG, B16, C17, ONE, TIE, NOBODY = 0, 1, 2, 3, 4, 5
J0, JT, NOTHING = 0, MI - 2, MI - 1
_MERGE = {}


def merge_problem():
    if "p" not in _MERGE:
        rng = np.random.default_rng(2024)
        rows = []
        for u, n in ((LONG, 4200), (B16, 2048), (C17, 2049), (ONE, 1)):
            rows += [(u, int(j)) for j in rng.choice(np.arange(1, MI - 2), n, replace=False)]
        rows += [(u, J0) for u in range(10, 50)]
        tu = np.array([r[0] for r in rows], np.int32)
        ti = np.array([r[1] for r in rows], np.int32)
        tr = rng.integers(1, 6, tu.size).astype(np.float32)
        perm = rng.permutation(tu.size)
        tu, ti, tr = tu[perm], ti[perm], tr[perm]
        # the tied rows last, so their list positions ascend with the train row
        tu = np.append(tu, np.full(130, TIE, np.int32))
        ti = np.append(ti, np.full(130, JT, np.int32))
        tr = np.append(tr, np.full(130, 3.0, np.float32))
        qs = [(NOBODY, NOTHING),                      # 0 slots: no candidate at all
              (ONE, NOTHING),                          # 1 slot
              (NOBODY, J0),                            # 1 slot, item side
              (B16, NOTHING),                          # 16 slots: one full round of the row
              (C17, NOTHING), (B16, J0),               # 17: lane 0's second round
              (LONG, NOTHING), (LONG, J0),             # 33 and 34: past the unrolled rounds
              (12, J0),                                # a train pair (coupled), 2 slots
              (TIE, NOTHING), (NOBODY, JT),            # equal candidates in two slots, either side
              (TIE, JT)]                               # ... on both sides at once (coupled)
        qu, qi = np.array([q[0] for q in qs], np.int32), np.array([q[1] for q in qs], np.int32)
        _MERGE["p"] = dict(train=(tu, ti, tr), params=synth.mf_params(MU, MI, K16, 5), qu=qu, qi=qi)
    return _MERGE["p"]


def merge_oracle():
    from oracle import fia_oracle as fo
    P = merge_problem()
    if "want" not in _MERGE:
        tu, ti, tr = P["train"]
        ex = fo.CsrExact("MF", P["params"], K16, tu, ti, tr, WD, DAMPING)
        _MERGE["want"] = [ex.query(int(u), int(i)) for u, i in zip(P["qu"], P["qi"])]
    return _MERGE["want"]


def merge_run(K):
    P = merge_problem()
    m = RawModel("MF", K16, MU, MI, P["train"], P["params"])
    res = run(m, P["qu"], P["qi"], K=K)
    m.close()
    return res


def test_merge_row_slot_counts():
    """Queries with 0, 1, 16, 17, 33 and 34 candidate slots: top-1 position, train row and value
    against the oracle; the query without candidates reports -1 / -1 / NaN."""
    P, want = merge_problem(), merge_oracle()
    tu, ti, _ = P["train"]
    deg_u, deg_i = np.bincount(tu, minlength=MU), np.bincount(ti, minlength=MI)
    slots = (deg_u[P["qu"]] + 127) // 128 + (deg_i[P["qi"]] + 127) // 128
    assert {0, 1, 16, 17, 33, 34} <= set(int(s) for s in slots), slots
    res = merge_run(1)
    check_against_oracle(res, want, 1, "merge row")
    assert res["topk_pos"][0, 0] == -1 and res["topk_idx"][0, 0] == -1 and np.isnan(res["topk_val"][0, 0])


def test_merge_row_tie_lower_position_wins():
    """130 train rows with the same user, item and rating: the candidates of their two chunks
    carry the same key, and the lower related position wins -- position 0 on the user side
    (TIE with an unrated item), on the item side (JT with a user without ratings), and with
    both sides present (the pair itself: the user-side copy comes first)."""
    P = merge_problem()
    res = merge_run(1)
    tu, ti, _ = P["train"]
    first_row = int(np.nonzero((tu == TIE) & (ti == JT))[0][0])
    for q in (9, 10, 11):
        b, e = res["offsets"][q], res["offsets"][q + 1]
        infl = res["influence"][b:e]
        assert e - b == (260 if q == 11 else 130)
        assert np.array_equal(infl.view(np.int64), np.full(e - b, infl.view(np.int64)[0])), q
        assert res["topk_pos"][q, 0] == 0, (q, res["topk_pos"][q])
        assert res["topk_idx"][q, 0] == first_row, (q, res["topk_idx"][q])


def test_merge_row_batch_size_threshold():
    """The row per query serves batches of up to 16,384 queries, the thread per query larger
    ones.  16,384 queries of the 600 x 40 problem (1,024 workgroups of rows; a twentieth
    coupled) against the oracle; then the same queries and one more -- the other kernel -- give
    the same top-1 bits for all of them."""
    rng = np.random.default_rng(16384)
    P = problem()
    Q = 16384
    pairs = [P["free"][j] for j in rng.integers(0, len(P["free"]), Q - Q // 20)]
    pairs += [P["train_pairs"][j] for j in rng.integers(0, len(P["train_pairs"]), Q // 20)]
    qu, qi = arrays(pairs)
    order = np.argsort(qi, kind="stable")
    qu, qi = qu[order], qi[order]
    m = model()
    at = run(m, qu, qi, K=1)
    check_against_oracle(at, oracle_for(qu, qi), 1, "merge row Q=16384")
    past = run(m, np.append(qu, qu[:1]), np.append(qi, qi[:1]), K=1)
    for name in ("topk_pos", "topk_idx", "topk_val"):
        same_bits({name: at[name]}, {name: past[name][:Q]})
        same_bits({name: past[name][Q:]}, {name: at[name][:1]})
    m.close()


def test_merge_k2_other_path():
    """K = 2 on the same data: the thread-per-query merge, unchanged."""
    res = merge_run(2)
    check_against_oracle(res, merge_oracle(), 2, "merge K=2")
    assert (res["topk_pos"][9] == [0, 1]).all() and (res["topk_pos"][10] == [0, 1]).all()
