"""GPU tests of fia_edit_influence / get_edit_influence: the joint Newton effect of train rows
removed and hypothetical ratings added together,

    edit = v . (H - H_R + H_A)^-1 (b_R - b_A),   first_order = (H^-1 v) . (b_R - b_A)

against edit_reference (tests/test_edit_cpu.py: the definition in numpy, one solve per group, from
the fp64 oracle), against the two calls it generalises (get_group_influence with no additions,
get_candidate_newton_batch with one addition and no removal), and for the properties of the call:
joint is not the sum of singles, a rating replaced by itself, members that change no bit, bad
members, top-K, reproducibility under every rearrangement of the batch, the prepare_for cover and
the unsupported sizes.

Tolerance: the project's RTOL = 1e-5 relative to the largest |want| of the query (rel_err).  Both
sides work in fp64; every group is asserted on the CPU (tests/test_edit_cpu.py, and again here) to
give cond(H - H_R + H_A) < 1e8, none skipped.

The problem and the queries are those of tests/test_newton_cpu.py; every live query gets the
groups of edit_groups: empty, removal-only of 1 and 17 members, addition-only of 1, 2, 16 and 17
members mixing user side, item side and neither, a mixed group of 20 + 20, a related rating
replaced by another y, and a `both` addition (on a train-row query as the replacement of its own
row).  The n_q = 0 query gets two groups (NaN); the first query repeated at the end of the batch
gets the first query's groups.  The batch goes through Context.edit_influence: the facade refuses
bad members on the host."""
import numpy as np
import pytest

from influence import synth
from influence._lib import FIAError
from test_cand_newton_cpu import COND_MAX, SIZES, params_for
from test_edit_cpu import NO_ADDS, edit_groups, live_queries, reference_of, related_rows
from test_group_cpu import w3g_of
from test_gpu_parity import RTOL, make_model, rel_err
from test_newton_cpu import DAMP, I, U, WD, problem, queries

pytestmark = pytest.mark.gpu

NO_ROWS = np.zeros(0, np.int64)


class Case(object):
    pass


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def flatten(groups):
    """groups[q]: list of (remove_rows, add_triples) -> the call's seven arrays."""
    go, ro, ao, rows, adds = [0], [0], [0], [NO_ROWS], [NO_ADDS]
    for per_query in groups:
        for rem, add in per_query:
            rows.append(np.asarray(rem, np.int64))
            adds.append(np.asarray(add, np.float64).reshape(-1, 3))
            ro.append(ro[-1] + rows[-1].size)
            ao.append(ao[-1] + adds[-1].shape[0])
        go.append(len(ro) - 1)
    add = np.concatenate(adds)
    return (np.array(go, np.int64), np.array(ro, np.int64), np.concatenate(rows).astype(np.int32),
            np.array(ao, np.int64), add[:, 0].astype(np.int32), add[:, 1].astype(np.int32), add[:, 2].astype(np.float32))


def run(c, qs, groups, K=0, edit=True, first=True, dtheta=True):
    """One call through the binding: dict(edit [G], first [G], dtheta [G, D], pos [Q, K], val [Q, K])."""
    import torch
    ctx = c.m.ctx
    dev = ctx.torch_device
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)
    go, ro, rr, ao, au, ai, ay = flatten(groups)
    Q, G, D = len(qs), ro.size - 1, c.D
    qu, qi = t([q[0] for q in qs], np.int32), t([q[1] for q in qs], np.int32)
    full = lambda n: torch.full((max(n, 1),), 7.0, dtype=torch.float64, device=dev)
    ed = full(G) if edit else None
    fo = full(G) if first else None
    dth = full(G * D) if dtheta else None
    tp = torch.full((Q * K,), -7, dtype=torch.int64, device=dev) if K else None
    tv = torch.full((Q * K,), 7.0, dtype=torch.float64, device=dev) if K else None
    ctx.edit_influence(qu, qi, t(go, np.int64), t(ro, np.int64), t(rr, np.int32), t(ao, np.int64), t(au, np.int32),
                       t(ai, np.int32), t(ay, np.float32), ed, fo, dth, K, tp, tv)
    return dict(go=go, edit=ed[:G].cpu().numpy() if edit else None, first=fo[:G].cpu().numpy() if first else None,
                dtheta=dth[:G * D].cpu().numpy().reshape(G, D) if dtheta else None,
                pos=tp.cpu().numpy().reshape(Q, K) if K else None, val=tv.cpu().numpy().reshape(Q, K) if K else None)


def same_bits(a, b, sel_a=slice(None), sel_b=slice(None)):
    return all(np.array_equal(bits(a[k][sel_a]), bits(b[k][sel_b])) for k in ("edit", "first", "dtheta"))


@pytest.fixture(scope="module", params=SIZES, ids=lambda v: "%s-k%d" % v)
def case(request, tmp_path_factory):
    from oracle import fia_oracle as fo
    model, k = request.param
    c = Case()
    c.model, c.k = model, k
    c.tu, c.ti, c.tr = tu, ti, tr = problem()
    c.p = params_for(model, k)
    c.W3g = w3g_of(model, c.p, k)
    c.qs = queries(tu, ti)
    c.Q = len(c.qs)
    c.D = 2 * k + 2 if model == "MF" else 4 * k
    qu = np.array([q[0] for q in c.qs], np.int32)
    qi = np.array([q[1] for q in c.qs], np.int32)
    c.m = make_model(model, U, I, k, (tu, ti, tr), (qu, qi), c.p, wd=WD, damping=DAMP,
                     tmpdir=tmp_path_factory.mktemp("edit_%s%d" % (model, k)))
    live = live_queries(tu, ti)
    c.cores = {q: fo.query(model, c.p, k, tu, ti, tr, q[0], q[1], WD, DAMP) for q in live}
    c.names, c.groups = [], []
    for (u, i) in c.qs:
        if (u, i) in c.cores:
            gs = edit_groups(tu, ti, tr, u, i, 90 + live.index((u, i)))
        else:                                           # n_q = 0
            gs = [("rem", np.array([0, 1], np.int64), NO_ADDS), ("add", NO_ROWS, np.array([[u, 3, 2.5]]))]
        c.names.append([g[0] for g in gs])
        c.groups.append([g[1:] for g in gs])
    # the reference, once: NaN exactly at the n_q = 0 query
    G = sum(len(g) for g in c.groups)
    c.want = dict(edit=np.full(G, np.nan), first=np.full(G, np.nan), dtheta=np.full((G, c.D), np.nan))
    c.cond = 0.0
    g = 0
    for q, (u, i) in enumerate(c.qs):
        for rem, add in c.groups[q]:
            if (u, i) in c.cores:
                ref = reference_of(model, c.p, k, c.cores[(u, i)], u, i, rem, add, c.W3g)
                c.want["edit"][g], c.want["first"][g], c.want["dtheta"][g] = ref["edit"], ref["first_order"], ref["dtheta"]
                c.cond = max(c.cond, ref["cond"])
            g += 1
    c.base = run(c, c.qs, c.groups, K=4)
    c.go = c.base["go"]
    yield c
    c.m.ctx.close()


def span(c, q):
    return slice(int(c.go[q]), int(c.go[q + 1]))


def group_of(c, q, name):
    return int(c.go[q]) + c.names[q].index(name)


def test_matches_reference(case):
    """Every group of every query against the per-group solve, none excluded; +0.0 at the empty
    groups; NaN exactly at the n_q = 0 query."""
    c = case
    assert c.cond < COND_MAX, c.cond
    nan = np.isnan(c.want["edit"])
    assert nan.sum() == 2 and nan[span(c, 5)].all()
    for key in ("edit", "first"):
        assert np.array_equal(np.isnan(c.base[key]), nan), key
    assert np.array_equal(np.isnan(c.base["dtheta"]), np.isnan(c.want["dtheta"]))
    worst = {}
    for q in range(c.Q):
        if q == 5:
            continue
        for key in ("edit", "first", "dtheta"):
            err = rel_err(c.base[key][span(c, q)], c.want[key][span(c, q)])
            print("query %s %s: rel err %.2e (largest |want| %.3e)" % (
                c.qs[q], key, err, np.abs(c.want[key][span(c, q)]).max()))
            worst[key] = max(worst.get(key, 0.0), err)
            assert err < RTOL, (c.qs[q], key, err)
        g = group_of(c, q, "empty")
        for key in ("edit", "first", "dtheta"):
            assert (bits(c.base[key][g]) == 0).all(), (c.qs[q], key)
    print("largest rel err %s, largest cond %.3e" % (worst, c.cond))


def test_no_additions_is_the_group_call(case):
    c = case
    live = [q for q in range(c.Q - 1) if q != 5]
    res = c.m.get_group_influence(live, [[c.groups[q][c.names[q].index(n)][0] for n in ("rem1", "rem17")]
                                         for q in live])
    for j, q in enumerate(live):
        mine = np.array([c.base["edit"][group_of(c, q, n)] for n in ("rem1", "rem17")])
        first = np.array([c.base["first"][group_of(c, q, n)] for n in ("rem1", "rem17")])
        sl = slice(int(res["grp_offsets"][j]), int(res["grp_offsets"][j + 1]))
        scale = np.abs(c.want["edit"][span(c, q)]).max()
        assert np.abs(mine - res["group"][sl]).max() < RTOL * scale, c.qs[q]
        assert np.abs(first - res["first_order"][sl]).max() < RTOL * np.abs(c.want["first"][span(c, q)]).max()


def test_one_addition_is_minus_the_candidate_call(case):
    c = case
    live = [q for q in range(c.Q - 1) if q != 5]
    names = [("add1", "replace_own" if "replace_own" in c.names[q] else "add_both") for q in live]
    X, Y, singles = [], [], []
    for q, (n1, n2) in zip(live, names):
        a1 = c.groups[q][c.names[q].index(n1)][1][0]
        a2 = c.groups[q][c.names[q].index(n2)][1][0]    # the `both` addition, alone here
        X += [a1[:2], a2[:2]]
        Y += [a1[2], a2[2]]
        singles.append([(NO_ROWS, a1[None, :]), (NO_ROWS, a2[None, :])])
    got = run(c, [c.qs[q] for q in live], singles)
    res = c.m.get_candidate_newton_batch(live, np.arange(0, 2 * len(live) + 1, 2), np.array(X, np.int64),
                                         np.array(Y, np.float32))
    for j, q in enumerate(live):
        scale = max(np.abs(c.want["edit"][span(c, q)]).max(), np.abs(res["newton"][2 * j:2 * j + 2]).max())
        assert np.abs(got["edit"][2 * j:2 * j + 2] + res["newton"][2 * j:2 * j + 2]).max() < RTOL * scale, c.qs[q]
        assert bits(got["edit"][2 * j:2 * j + 1])[0] == bits(c.base["edit"][group_of(c, q, "add1"):][:1])[0]


def test_joint_is_not_the_sum_of_singles(case):
    """The 16 additions of user 0's train-row query, together and one by one."""
    c = case
    add = c.groups[0][c.names[0].index("add16")][1]
    singles = run(c, c.qs[:1], [[(NO_ROWS, add[j:j + 1]) for j in range(16)]])["edit"]
    joint = c.base["edit"][group_of(c, 0, "add16")]
    want_singles = np.array([reference_of(c.model, c.p, c.k, c.cores[c.qs[0]], 0, c.qs[0][1], NO_ROWS, add[j:j + 1],
                                          c.W3g)["edit"] for j in range(16)])
    assert rel_err(singles, want_singles) < RTOL
    ref_gap = abs(c.want["edit"][group_of(c, 0, "add16")] - want_singles.sum()) / np.abs(want_singles).max()
    gap = abs(joint - singles.sum()) / np.abs(singles).max()
    print("|edit - sum of singles| / largest |single|: %.3e (reference %.3e)" % (gap, ref_gap))
    assert gap > 100 * RTOL, gap


def test_replaced_by_itself_is_nothing(case):
    """Remove an ordinary related row and add the same (a, b, y): the edit vanishes against the
    removal alone."""
    c = case
    qsel = [0, 1, 6]
    groups = []
    for q in qsel:
        j = int(c.groups[q][c.names[q].index("replace")][0][0])
        same = np.array([[c.tu[j], c.ti[j], c.tr[j]]], np.float64)
        groups.append([(np.array([j]), NO_ADDS), (np.array([j]), same)])
    got = run(c, [c.qs[q] for q in qsel], groups)
    for t in range(len(qsel)):
        alone, both = got["edit"][2 * t], got["edit"][2 * t + 1]
        assert alone != 0.0 and abs(both) < RTOL * abs(alone), (c.qs[qsel[t]], alone, both)


def test_members_that_change_no_bit(case):
    """An m_j = 0 removal appended to a group changes no bit; a group of only such removals is +0.0."""
    c = case
    qsel = [0, 4, 8]
    groups, plain = [], []
    for q in qsel:
        _, unrel = related_rows(c.tu, c.ti, *c.qs[q])
        rem, add = c.groups[q][c.names[q].index("mixed")]
        free = np.array([r for r in unrel if r not in rem], np.int64)
        groups.append([(np.concatenate([rem, free[:1]]), add), (free[:3], NO_ADDS),
                       (np.concatenate([free[1:2], rem]), add)])
        plain.append(group_of(c, q, "mixed"))
    got = run(c, [c.qs[q] for q in qsel], groups)
    for t, g in enumerate(plain):
        for key in ("edit", "first", "dtheta"):
            assert np.array_equal(bits(got[key][3 * t]), bits(c.base[key][g])), (qsel[t], key)
            assert np.array_equal(bits(got[key][3 * t + 2]), bits(c.base[key][g])), (qsel[t], key)
            assert (bits(got[key][3 * t + 1]) == 0).all(), (qsel[t], key)


def test_bad_members_spoil_their_own_group_only(case):
    c = case
    q = 0
    per = list(c.groups[q])
    n_train = c.tu.size
    rem, add = per[c.names[q].index("mixed")]
    bad = [(np.concatenate([rem[:5], [n_train], rem[5:]]), add),
           (np.concatenate([[-1], rem]), NO_ADDS),
           (rem, np.concatenate([add[:7], [[U, 3, 2.5]], add[7:]])),
           (NO_ROWS, np.array([[0, -1, 2.5]])),
           (NO_ROWS, np.array([[-3, I, 2.5]]))]
    mixed = []
    for j, g in enumerate(per):                         # a bad group between every two good ones
        mixed.append(g)
        mixed.append(bad[j % len(bad)])
    got = run(c, [c.qs[q], c.qs[1]], [mixed, c.groups[1]])
    n = len(per)
    for key in ("edit", "first", "dtheta"):
        assert np.isnan(got[key][1:2 * n:2]).all(), key
        assert np.array_equal(bits(got[key][0:2 * n:2]), bits(c.base[key][span(c, q)])), key
        assert np.array_equal(bits(got[key][2 * n:]), bits(c.base[key][span(c, 1)])), key


def test_query_id_out_of_range(case):
    """Through the binding: NaN for its groups, the neighbours' bits unchanged."""
    c = case
    for badq in ((U, 3), (0, -1), (-2, I + 5)):
        got = run(c, [c.qs[0], badq, c.qs[4]], [c.groups[0], c.groups[4], c.groups[4]], K=2)
        n0, n4 = len(c.groups[0]), len(c.groups[4])
        for key in ("edit", "first", "dtheta"):
            assert np.isnan(got[key][n0:n0 + n4]).all(), (badq, key)
            assert np.array_equal(bits(got[key][:n0]), bits(c.base[key][span(c, 0)])), (badq, key)
            assert np.array_equal(bits(got[key][n0 + n4:]), bits(c.base[key][span(c, 4)])), (badq, key)
        assert np.array_equal(got["pos"][1], [0, 1]) and np.isnan(got["val"][1]).all()   # all NaN, in order
        assert np.array_equal(got["pos"][0], c.base["pos"][0][:2])


def check_topk(pos, val, full, K):
    """|value| descending, position ascending, NaN last; -1 / NaN in unused slots; the bits of the
    full values."""
    key = np.where(np.isnan(full), -1.0, np.abs(full))
    order = np.argsort(-key, kind="stable")[:K]
    m = order.size
    assert np.array_equal(pos[:m], order)
    assert np.array_equal(bits(val[:m]), bits(full[order]))
    assert (pos[m:] == -1).all() and np.isnan(val[m:]).all()


@pytest.mark.parametrize("K", [1, 4])
def test_topk(case, K):
    """Per query over its groups; a query with fewer groups than K, and one with none."""
    c = case
    qs = c.qs + [c.qs[2], c.qs[3]]
    groups = c.groups + [c.groups[2][1:3], []]
    got = run(c, qs, groups, K=K)
    assert np.array_equal(bits(got["edit"][:c.go[-1]]), bits(c.base["edit"]))
    lean = run(c, qs, groups, K=K, edit=False, first=False, dtheta=False)       # top-K only
    assert np.array_equal(lean["pos"], got["pos"]) and np.array_equal(bits(lean["val"]), bits(got["val"]))
    assert got["pos"].shape == (len(qs), K) and got["pos"].dtype == np.int64
    for q in range(len(qs)):
        check_topk(got["pos"][q], got["val"][q], got["edit"][got["go"][q]:got["go"][q + 1]], K)
    assert (got["pos"][-1] == -1).all() and np.isnan(got["val"][-1]).all()     # no groups
    if K == 4:
        assert np.array_equal(got["pos"][:c.Q], c.base["pos"]) and (got["pos"][-2][2:] == -1).all()
        assert np.array_equal(bits(got["val"][:c.Q]), bits(c.base["val"]))


def test_reproducible_under_rearrangement(case):
    """A second call, the query repeated at the end of the batch, the groups permuted within a
    query and the queries permuted: the same bits."""
    c = case
    again = run(c, c.qs, c.groups, K=4)
    assert same_bits(again, c.base)
    assert np.array_equal(again["pos"], c.base["pos"]) and np.array_equal(bits(again["val"]), bits(c.base["val"]))
    assert c.qs[-1] == c.qs[0] and same_bits(c.base, c.base, span(c, c.Q - 1), span(c, 0))
    rng = np.random.default_rng(12)
    # the groups permuted within every query
    perms = [rng.permutation(len(g)) for g in c.groups]
    got = run(c, c.qs, [[g[j] for j in p] for g, p in zip(c.groups, perms)])
    take = np.concatenate([c.go[q] + p for q, p in enumerate(perms)]).astype(np.int64)
    assert same_bits(got, c.base, slice(None), take)
    # the queries permuted, each with its groups
    perm = rng.permutation(c.Q)
    got = run(c, [c.qs[q] for q in perm], [c.groups[q] for q in perm])
    take = np.concatenate([np.arange(c.go[q], c.go[q + 1]) for q in perm]).astype(np.int64)
    assert same_bits(got, c.base, slice(None), take)


def test_argument_checks_through_the_binding(case):
    """Counts above 2^31 - 1, K out of range or with null top-K arrays, and no output requested:
    FIA_ERR_INVALID before anything is reserved or launched (the arrays passed are never read);
    no queries: FIA_OK."""
    import torch
    ctx = case.m.ctx
    dev = ctx.torch_device
    q = torch.zeros(1, dtype=torch.int32, device=dev)
    off = torch.zeros(2, dtype=torch.int64, device=dev)
    f = torch.zeros(1, dtype=torch.float32, device=dev)
    d = torch.zeros(1, dtype=torch.float64, device=dev)
    p = lambda t: t.data_ptr()
    fn = ctx.lib.fia_edit_influence
    call = lambda G=0, TR=0, TA=0, ed=None, K=0, tp=None, tv=None, Q=1: fn(
        ctx.h, Q, p(q), p(q), p(off), G, p(off), TR, p(q), p(off), TA, p(q), p(q), p(f), ed, None, None, K, tp, tv, None)
    assert call(G=2 ** 31, ed=p(d)) == 1
    assert call(TR=2 ** 31, ed=p(d)) == 1
    assert call(TA=2 ** 31, ed=p(d)) == 1
    assert call(ed=p(d), K=65) == 1 and call(ed=p(d), K=-1) == 1
    assert call(ed=p(d), K=4) == 1                      # null top-K arrays
    assert call() == 1                                  # nothing asked for
    assert call(ed=p(d)) == 0 and call(ed=p(d), Q=0) == 0


def test_facade_matches_the_binding(case):
    c = case
    qsel = [0, 4, 7, 10]
    res = c.m.get_edit_influence(qsel, [c.groups[q] for q in qsel], K=3, dtheta=True)
    take = np.concatenate([np.arange(c.go[q], c.go[q + 1]) for q in qsel]).astype(np.int64)
    assert np.array_equal(res["grp_offsets"], np.concatenate([[0], np.cumsum([len(c.groups[q]) for q in qsel])]))
    assert np.array_equal(bits(res["edit"]), bits(c.base["edit"][take]))
    assert np.array_equal(bits(res["first_order"]), bits(c.base["first"][take]))
    assert np.array_equal(bits(res["dtheta"]), bits(c.base["dtheta"][take]))
    for j in range(len(qsel)):
        check_topk(res["topk_pos"][j], res["topk_val"][j],
                   res["edit"][res["grp_offsets"][j]:res["grp_offsets"][j + 1]], 3)
    lean = c.m.get_edit_influence(qsel, [c.groups[q] for q in qsel], first_order=False)
    assert lean["first_order"] is None and lean["dtheta"] is None and lean["topk_pos"] is None
    assert np.array_equal(bits(lean["edit"]), bits(res["edit"]))


def test_cover_independent(case):
    """After prepare_for on the queries alone -- the members' entities mostly outside it -- the
    results are bitwise those after the full prepare.  Runs last on the model."""
    c = case
    live = [q for q in range(c.Q) if q != 5]
    c.m.prepare_for(live)
    try:
        sub = run(c, c.qs, c.groups, K=4)
    finally:
        c.m.ctx.prepare()
    assert same_bits(sub, c.base)
    assert np.array_equal(sub["pos"], c.base["pos"]) and np.array_equal(bits(sub["val"]), bits(c.base["val"]))


def test_large_k_is_unsupported(tmp_path):
    """The large-k models: FIA_ERR_UNSUPPORTED through the facade, with a text that says so."""
    tu, ti, tr = problem()
    qs = queries(tu, ti)[:2]
    qu = np.array([q[0] for q in qs], np.int32)
    qi = np.array([q[1] for q in qs], np.int32)
    m = make_model("MF", U, I, 128, (tu, ti, tr), (qu, qi), synth.mf_params(U, I, 128, 3), wd=WD, damping=DAMP,
                   tmpdir=tmp_path)
    try:
        with pytest.raises(FIAError, match="unsupported.*large-k"):
            m.get_edit_influence([0, 1], [[(np.array([0]), [(0, 1, 2.5)])], []], K=1)
    finally:
        m.ctx.close()
