"""GPU tests of fia_group_influence / get_group_influence: the predicted change of r-hat(u, i)
when a SET of train rows is removed together,

    dtheta = (H - H_S)^-1 b_S,  group = v . dtheta,  first_order = (H^-1 v) . b_S

against group_reference (tests/test_group_cpu.py), the definition restated in numpy from the
fp64 oracle's per-query H, G, e and x, and for the properties of the call: empty groups and
unrelated rows, position independence, determinism, bad rows, n_q = 0, the prepare_for cover.

Tolerance: the project's RTOL = 1e-5 relative to the largest |want| (rel_err), for group and
first_order over the batch and for dtheta per group.  Both sides solve in fp64, so the error is
about eps * cond(H - H_S): every tested group is asserted (on the CPU) to leave a system with
condition number below 1e8, which keeps that bound under 1e-7.

The problem: 12 users, 128 items, 418 ratings.  User 0 rates items 0 .. 125 (so that half of
its list and half of an item's list are more than one wave width of members), users 1 .. 9 rate
32 or 33 of items 0 .. 39, (3, 5) is present twice, user 10 has three ratings, user 11 and items
126 and 127 have none; rows are shuffled."""
import numpy as np
import pytest

from influence import synth
from test_group_cpu import group_reference, w3g_of
from test_gpu_parity import RTOL, make_model, rel_err

pytestmark = pytest.mark.gpu

WD, DAMP = 1e-3, 1e-6
U, I = 12, 128
HEAVY = 126
DUP = (3, 5)
SIZES = [("MF", 8), ("MF", 16), ("MF", 32), ("MF", 64), ("NCF", 8), ("NCF", 16), ("NCF", 32)]
COND_MAX = 1e8


def problem():
    rng = np.random.default_rng(21)
    rows = [(0, b) for b in range(HEAVY)]
    for a in range(1, 10):
        items = [int(b) for b in rng.choice(40, 32, replace=False)]
        if a == DUP[0]:
            items = [b for b in items if b != DUP[1]][:31] + [DUP[1], DUP[1]]
        rows += [(a, b) for b in items]
    rows += [(10, 1), (10, 2), (10, 41)]
    tu = np.array([r[0] for r in rows], np.int32)
    ti = np.array([r[1] for r in rows], np.int32)
    tr = (rng.random(len(rows)) * 4.0 + 1.0).astype(np.float32)
    perm = rng.permutation(len(rows))                   # a train row is not its list position
    tu, ti, tr = tu[perm], ti[perm], tr[perm]
    d = np.nonzero((tu == DUP[0]) & (ti == DUP[1]))[0]
    assert d.size == 2 and tr[d[0]] != tr[d[1]]
    assert (tu == 0).sum() == HEAVY > 64 and (tu == 11).sum() == 0 and (ti >= HEAVY).sum() == 0
    return tu, ti, tr


# the queries: a train row of the heavy user; the duplicated pair; the heavy user with an
# unrated item (user side only); user 11 (no ratings) with a rated item (item side only); the
# duplicated pair's user with an item it has not rated (no train row); n_q = 0; and again the
# first pair, later in the batch
def queries(tu, ti):
    i0 = 7
    assert ((tu == 0) & (ti == i0)).sum() == 1 and (ti == i0).sum() >= 6
    i4 = next(b for b in range(40) if not ((tu == DUP[0]) & (ti == b)).any() and (ti == b).sum() >= 4)
    return [(0, i0), DUP, (0, 126), (11, i0), (DUP[0], i4), (11, 127), (0, i0)]


def rows_of(tu, ti, u=None, i=None):
    m = np.ones(len(tu), bool)
    if u is not None:
        m &= tu == u
    if i is not None:
        m &= ti == i
    return np.nonzero(m)[0]


def build_groups(tu, ti, qs):
    """groups[q]: a list of (name, rows).  No group removes more than half of either side."""
    rng = np.random.default_rng(8)
    pick = lambda rows, n: np.sort(rng.choice(rows, n, replace=False))
    (u0, i0) = qs[0]
    own = rows_of(tu, ti, u0, i0)
    user_side = np.setdiff1d(rows_of(tu, ti, u=u0), own)
    item_side = np.setdiff1d(rows_of(tu, ti, i=i0), own)
    unrelated = np.nonzero((tu != u0) & (ti != i0))[0]
    n_item = item_side.size // 2
    g0 = [("one", user_side[:1]),
          ("user", pick(user_side, 7)),
          ("item", pick(item_side, n_item)),
          ("mixed", np.concatenate([pick(user_side, 9), pick(item_side, n_item)])),
          ("own", np.concatenate([own, pick(user_side, 3)])),
          ("twenty", pick(user_side, 20)),              # the RQ1-sized group of the issue
          ("wide", np.concatenate([pick(item_side, n_item), pick(user_side, 62)])),    # > 64, all related
          ("empty", np.zeros(0, np.int64)),
          ("user+unrelated", None)]                     # filled below: "user" with unrelated rows mixed in
    user_rows = g0[1][1]
    mixed_in = np.concatenate([unrelated[:3], user_rows[:4], unrelated[3:70], user_rows[4:], unrelated[70:75]])
    g0[-1] = ("user+unrelated", mixed_in)
    assert mixed_in.size > 64 and g0[6][1].size > 64
    dup_rows = rows_of(tu, ti, *DUP)
    u3 = np.setdiff1d(rows_of(tu, ti, u=DUP[0]), dup_rows)
    i5 = np.setdiff1d(rows_of(tu, ti, i=DUP[1]), dup_rows)
    g1 = [("dup-one", dup_rows[:1]),                    # one of the two rows of the pair: m = 2
          ("dup-both+", np.concatenate([dup_rows, pick(u3, 5), pick(i5, max((i5.size + 2) // 2 - 2, 0))]))]
    g2 = [("user-only-query", pick(rows_of(tu, ti, u=0), 30)),
          ("one", rows_of(tu, ti, u=0)[5:6])]
    it = rows_of(tu, ti, i=i0)
    g3 = [("item-only-query", pick(it, it.size // 2))]
    (u4, i4) = qs[4]
    ru = np.setdiff1d(rows_of(tu, ti, u=u4), dup_rows)
    it4 = rows_of(tu, ti, i=i4)
    # the two rows of the duplicated pair as user-side members (m = 1 each) of another query
    g4 = [("mixed", np.concatenate([pick(ru, 10), pick(it4, it4.size // 2)])),
          ("with-dup", np.concatenate([dup_rows[:1], pick(ru, 4), dup_rows[1:], pick(it4, 1)]))]
    g5 = [("nq0", user_side[:3]), ("nq0-empty", np.zeros(0, np.int64))]
    g6 = [("user", user_rows)]                          # g0's "user" group, at another place
    return [g0, g1, g2, g3, g4, g5, g6]


class Case(object):
    pass


@pytest.fixture(scope="module", params=SIZES, ids=lambda v: "%s-k%d" % v)
def case(request, tmp_path_factory):
    from oracle import fia_oracle as fo
    model, k = request.param
    c = Case()
    c.model, c.k = model, k
    c.tu, c.ti, c.tr = tu, ti, tr = problem()
    c.p = synth.mf_params(U, I, k, 3) if model == "MF" else synth.ncf_params(U, I, k, 3)
    c.qs = queries(tu, ti)
    c.named = build_groups(tu, ti, c.qs)
    c.groups = [[np.asarray(r, np.int64) for _, r in per] for per in c.named]
    qu = np.array([q[0] for q in c.qs], np.int32)
    qi = np.array([q[1] for q in c.qs], np.int32)
    c.m = make_model(model, U, I, k, (tu, ti, tr), (qu, qi), c.p, wd=WD, damping=DAMP,
                     tmpdir=tmp_path_factory.mktemp("group_%s%d" % (model, k)))
    c.D = fo.num_params(model, k)
    W3g = w3g_of(model, c.p, k)
    c.cores = [fo.query(model, c.p, k, tu, ti, tr, u, i, WD, DAMP) for (u, i) in c.qs]
    # the reference, once: per group (query, name, reference or None where n_q = 0)
    c.refs = []
    for q, per in enumerate(c.named):
        for name, rows in per:
            ref = group_reference(c.cores[q], rows, WD, DAMP, W3g) if c.cores[q]["n"] else None
            c.refs.append((q, name, ref))
    c.res = c.m.get_group_influence(list(range(len(c.qs))), c.groups, return_dtheta=True)
    yield c
    c.m.ctx.close()


def gid(c, q, name):
    return next(g for g, (qq, nn, _) in enumerate(c.refs) if qq == q and nn == name)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def test_groups_are_well_conditioned(case):
    """The tested groups remove at most half of either side and leave cond(H - H_S) < 1e8, so
    RTOL is a meaningful bound (eps * cond < 1e-7)."""
    c = case
    worst = 0.0
    for (q, name, ref), rows in zip(c.refs, [r for per in c.groups for r in per]):
        if ref is None or rows.size == 0:
            continue
        u, i = c.qs[q]
        su, si = (c.tu == u).sum(), (c.ti == i).sum()
        assert (c.tu[rows] == u).sum() <= max(su // 2, 1) and (c.ti[rows] == i).sum() <= max(si // 2, 1), (q, name)
        worst = max(worst, ref["cond"])
        assert ref["cond"] < COND_MAX, (q, name, ref["cond"])
    print("largest cond(H - H_S) %.3e" % worst)


def test_matches_reference(case):
    """group, first_order and dtheta of every group: size 1, user side, item side, mixed, with
    the own pair (m = 2), with the duplicated pair, more than 64 members, 20 rows of the heavy
    user; queries with one side only."""
    c = case
    res = c.res
    G = len(c.refs)
    assert res["group"].shape == (G,) and res["first_order"].shape == (G,) and res["dtheta"].shape == (G, c.D)
    assert res["grp_offsets"].tolist() == np.cumsum([0] + [len(p) for p in c.groups]).tolist()
    live = [g for g, (_, _, ref) in enumerate(c.refs) if ref is not None]
    want_g = np.array([c.refs[g][2]["group"] for g in live])
    want_f = np.array([c.refs[g][2]["first_order"] for g in live])
    eg, ef = rel_err(res["group"][live], want_g), rel_err(res["first_order"][live], want_f)
    print("rel err group %.2e first_order %.2e (largest |want| %.3e)" % (eg, ef, np.abs(want_g).max()))
    assert np.isfinite(res["group"][live]).all() and np.isfinite(res["first_order"][live]).all()
    assert eg < RTOL and ef < RTOL
    worst = 0.0
    for g in live:
        err = rel_err(res["dtheta"][g], c.refs[g][2]["dtheta"])
        worst = max(worst, err)
        assert err < RTOL, (c.refs[g][:2], err)
    print("rel err dtheta %.2e" % worst)
    # the group of 20 of the issue: the corrected value is what the reference says, and it is
    # not the first-order sum (the curvature of 20 of ~100 ratings matters)
    g20 = gid(c, 0, "twenty")
    ref = c.refs[g20][2]
    print("20 of the heavy user: group %.6e first_order %.6e (reference %.6e / %.6e)" % (
        res["group"][g20], res["first_order"][g20], ref["group"], ref["first_order"]))
    assert abs(res["group"][g20] - ref["group"]) < RTOL * abs(ref["group"])
    assert abs(res["first_order"][g20] - ref["first_order"]) < RTOL * abs(ref["first_order"])
    assert abs(ref["group"] - ref["first_order"]) > 100 * RTOL * abs(ref["first_order"])


def test_first_order_is_the_sum_of_influences(case):
    """first_order = the sum of get_influence_batch's influence over the group's occurrences
    in the related list."""
    c = case
    batch = c.m.get_influence_batch(list(range(len(c.qs))), K=0, full=True)
    off = batch["offsets"]
    got, want = [], []
    for g, (q, name, ref) in enumerate(c.refs):
        if ref is None:
            continue
        rel = batch["rel_idx"][off[q]:off[q + 1]]
        infl = batch["influence"][off[q]:off[q + 1]]
        rows = [r for per in c.groups for r in per][g]
        got.append(c.res["first_order"][g])
        want.append(infl[np.isin(rel, rows)].sum())
    assert rel_err(np.array(got), np.array(want)) < RTOL


def test_empty_group_and_unrelated_rows(case):
    """An empty group is exactly +0.0 everywhere; a group with unrelated rows mixed in (more
    than 64 listed members) is bitwise the group alone."""
    c = case
    res = c.res
    ge = gid(c, 0, "empty")
    assert bits(res["group"][ge:ge + 1])[0] == 0 and bits(res["first_order"][ge:ge + 1])[0] == 0
    assert (bits(res["dtheta"][ge]) == 0).all()
    a, b = gid(c, 0, "user"), gid(c, 0, "user+unrelated")
    for key in ("group", "first_order", "dtheta"):
        assert np.array_equal(bits(res[key][a]), bits(res[key][b])), key
    assert res["group"][a] != 0.0


def test_position_independent_and_deterministic(case):
    """The same group of the same pair later in the batch, the batch reversed, and a second
    identical call: the same bits."""
    c = case
    res = c.res
    a, b = gid(c, 0, "user"), gid(c, 6, "user")
    for key in ("group", "first_order", "dtheta"):
        assert np.array_equal(bits(res[key][a]), bits(res[key][b])), key
    again = c.m.get_group_influence(list(range(len(c.qs))), c.groups, return_dtheta=True)
    for key in ("group", "first_order", "dtheta"):
        assert np.array_equal(bits(res[key]), bits(again[key])), key
    Q = len(c.qs)
    order = list(range(Q))[::-1]
    rev = c.m.get_group_influence(order, [c.groups[q][::-1] for q in order], return_dtheta=True)
    for key in ("group", "first_order", "dtheta"):
        assert np.array_equal(bits(rev[key][::-1]), bits(res[key])), key


def test_no_related_ratings_and_no_groups(case):
    """n_q = 0: NaN for the query's groups, the empty one included; a query without groups
    between two others changes nothing."""
    c = case
    res = c.res
    for name in ("nq0", "nq0-empty"):
        g = gid(c, 5, name)
        assert np.isnan(res["group"][g]) and np.isnan(res["first_order"][g]) and np.isnan(res["dtheta"][g]).all()
    groups = [c.groups[0], [], c.groups[2]]
    part = c.m.get_group_influence([0, 1, 2], groups, return_dtheta=True)
    assert part["grp_offsets"].tolist() == [0, len(groups[0]), len(groups[0]), len(groups[0]) + len(groups[2])]
    keep = list(range(len(c.groups[0]))) + [gid(c, 2, n) for n in ("user-only-query", "one")]
    for key in ("group", "first_order", "dtheta"):
        assert np.array_equal(bits(part[key]), bits(res[key][keep])), key
    none = c.m.get_group_influence([0, 1], [[], []])
    assert none["group"].shape == (0,) and none["first_order"].shape == (0,)


def test_out_of_range_row_through_the_binding(case):
    """A member row outside [0, n_train), given to Context.group_influence directly (the facade
    would refuse it): NaN for that group only, its neighbours keep their bits."""
    import torch
    c = case
    ctx = c.m.ctx
    dev = ctx.torch_device
    n_train = len(c.tr)
    user = c.groups[0][1]
    for bad_row in (n_train, -1, 2 ** 31 - 1):
        mem = [user, np.concatenate([user[:3], [bad_row], user[3:]]), user, np.array([bad_row]), user[:1]]
        mo = np.cumsum([0] + [len(r) for r in mem]).astype(np.int64)
        t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)
        qu, qi = t([c.qs[0][0]], np.int32), t([c.qs[0][1]], np.int32)
        G = len(mem)
        out = [torch.full((G,), 7.0, dtype=torch.float64, device=dev) for _ in range(2)]
        dth = torch.full((G * c.D,), 7.0, dtype=torch.float64, device=dev)
        ctx.group_influence(qu, qi, t([0, G], np.int64), t(mo, np.int64), t(np.concatenate(mem), np.int32),
                            out[0], out[1], dth)
        grp, fo_, dth = out[0].cpu().numpy(), out[1].cpu().numpy(), dth.cpu().numpy().reshape(G, c.D)
        for g in (1, 3):
            assert np.isnan(grp[g]) and np.isnan(fo_[g]) and np.isnan(dth[g]).all()
        a = gid(c, 0, "user")
        for g in (0, 2):
            assert bits(grp[g:g + 1])[0] == bits(c.res["group"][a:a + 1])[0]
            assert bits(fo_[g:g + 1])[0] == bits(c.res["first_order"][a:a + 1])[0]
            assert np.array_equal(bits(dth[g]), bits(c.res["dtheta"][a]))
        assert np.isfinite(grp[4]) and np.isfinite(dth[4]).all()


def test_cover_independent(case):
    """After prepare_for on the queries only, the results are bitwise those after the full
    prepare (member rows name users and items outside the cover).  Runs last on the model."""
    c = case
    Q = len(c.qs)
    live = [q for q in range(Q) if c.cores[q]["n"]]
    c.m.prepare_for(live)
    try:
        sub = c.m.get_group_influence(live, [c.groups[q] for q in live], return_dtheta=True)
    finally:
        c.m.ctx.prepare()
    keep = [g for g, (q, _, _) in enumerate(c.refs) if q in live]
    for key in ("group", "first_order", "dtheta"):
        assert np.array_equal(bits(sub[key]), bits(c.res[key][keep])), key
