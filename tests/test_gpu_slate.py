"""GPU tests of fia_count_related_slate / fia_slate_batch / get_slate_influence_batch: which ratings
shape a user's ranked list -- the influence of every rating of R_u ++ C_i1 ++ .. ++ C_im on
f = sum_l w_l r-hat(u, i_l), from ONE system over (theta_u, theta_i1 .. theta_im) --

    influence[offsets[q] + p] = x . (2 e_p g_p + wd M theta_t) / n,   x = H^-1 v

against slate_reference (tests/test_slate_cpu.py: the definition in numpy, row by row, checked there
against autograd, the pair reference and the oracle's single query), and for the properties of the
call: it equals the pair call at m = 2 and the single query at m = 1, it is not the weighted sum of
single queries, the bits (a second call, the batch reversed, outputs alone, the prepare_for cover),
a permuted slate, bad slates through the binding and the unsupported sizes.

Tolerance: the project's RTOL = 1e-5 relative to the largest |want| of the query (rel_err).  Both
sides work in fp64; every slate is asserted (tests/test_slate_cpu.py; the 64-item one here) to give
cond(H) < 1e8.

The problem is that of tests/test_newton_cpu.py (20 users x 320 items; user 0's 300 ratings cross a
256-position scoring tile; item lists of 1, 15, 16, 17 and about 10; a duplicated pair; empty
entities); the batch is slate_list's thirteen slates, all seven small-k sizes."""
import numpy as np
import pytest

from influence._lib import FIAError
from test_cand_newton_cpu import COND_MAX, params_for
from test_gpu_parity import RTOL, check_topk, make_model, rel_err
from test_newton_cpu import DAMP, I, U, WD, problem
from test_pair_cpu import SIZES as PAIR_SIZES
from test_slate_cpu import LONG, SIZES, slate_blocks, slate_list, slate_reference

pytestmark = pytest.mark.gpu

K = 4
EMPTY = 11                   # S11: n = 0, a finite value


class Case(object):
    pass


@pytest.fixture(scope="module", params=SIZES, ids=lambda v: "%s-k%d" % v)
def case(request, tmp_path_factory):
    model, k = request.param
    c = Case()
    c.model, c.k = model, k
    c.tu, c.ti, c.tr = tu, ti, tr = problem()
    c.p = params_for(model, k)
    c.sl = slate_list(tu, ti)
    c.Q = len(c.sl)
    c.users = [s[0] for s in c.sl]
    c.slates = [s[1] for s in c.sl]
    c.weights = [s[2] for s in c.sl]
    # the test rows of the calls compared against: S0 as the pair (0, 7) against 8, S1 and S9 as single queries
    c.rows = [(c.users[q], c.slates[q][0]) for q in (0, 1, 9)]
    c.m = make_model(model, U, I, k, (tu, ti, tr), (np.array([r[0] for r in c.rows], np.int32),
                                                    np.array([r[1] for r in c.rows], np.int32)), c.p,
                     wd=WD, damping=DAMP, tmpdir=tmp_path_factory.mktemp("slate_%s%d" % (model, k)))
    # the reference, once per distinct slate
    seen = {}
    for (u, items, w) in c.sl:
        key = (u, tuple(items), tuple(w))
        if key not in seen:
            seen[key] = slate_reference(model, c.p, k, tu, ti, tr, u, items, w, WD, DAMP)
    c.refs = [seen[(u, tuple(items), tuple(w))] for (u, items, w) in c.sl]
    c.base = c.m.get_slate_influence_batch(c.users, c.slates, c.weights, K=K, full=True)
    # a second call: the maximal slate, all 64 items rated by the user
    c.long_ref = slate_reference(model, c.p, k, tu, ti, tr, LONG[0], LONG[1], LONG[2], WD, DAMP)
    c.long = c.m.get_slate_influence_batch([LONG[0]], [LONG[1]], [LONG[2]], K=K, full=True)
    yield c
    c.m.ctx.close()


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def span(res, q):
    return slice(int(res["offsets"][q]), int(res["offsets"][q + 1]))


def same_query(a, qa, b, qb):
    """Every output of query qa of result a holds the bits of query qb of result b."""
    for key in ("influence", "rel_idx"):
        if key in a and key in b:
            assert np.array_equal(bits(a[key][span(a, qa)]), bits(b[key][span(b, qb)])), (key, qa, qb)
    for key in ("x", "value", "topk_val"):
        if key in a and key in b:
            assert np.array_equal(bits(a[key][qa]), bits(b[key][qb])), (key, qa, qb)
    for key in ("topk_pos", "topk_idx"):
        if key in a and key in b:
            assert np.array_equal(a[key][qa], b[key][qb]), (key, qa, qb)


def check_against(res, q, ref, what, worst):
    """Query q of a facade result against its reference: rel, influence, x, value, the top-K."""
    got = res["influence"][span(res, q)]
    assert np.array_equal(res["rel_idx"][span(res, q)], ref["rel"]), what
    assert res["x"][q].shape == ref["x"].shape
    pos = res["topk_pos"][q]
    if not ref["n"]:
        assert got.size == 0 and np.isnan(res["x"][q]).all()
        assert np.isfinite(res["value"][q]) and rel_err(res["value"][q:q + 1], np.array([ref["value"]])) < RTOL
        assert (pos == -1).all() and (res["topk_idx"][q] == -1).all() and np.isnan(res["topk_val"][q]).all()
        return 0
    errs = dict(influence=rel_err(got, ref["influence"]), x=rel_err(res["x"][q], ref["x"]),
                value=rel_err(res["value"][q:q + 1], np.array([ref["value"]])))
    print("%s n %d rel err influence %.2e x %.2e value %.2e (cond %.2e)" % (
        what, ref["n"], errs["influence"], errs["x"], errs["value"], ref["cond"]))
    for key, err in errs.items():
        worst[key] = max(worst[key], err)
        assert err < RTOL, (what, key, err)
    swaps = check_topk(pos, got, ref["influence"], K)
    m = min(K, ref["n"])
    assert np.array_equal(res["topk_idx"][q, :m], ref["rel"][pos[:m]])
    assert np.array_equal(bits(res["topk_val"][q, :m]), bits(got[pos[:m]]))
    assert (res["topk_idx"][q, m:] == -1).all() and np.isnan(res["topk_val"][q, m:]).all()
    return swaps


def test_matches_reference(case):
    c = case
    off = c.base["offsets"]
    assert off.tolist() == np.cumsum([0] + [r["n"] for r in c.refs]).tolist()
    assert c.base["influence"].shape == (off[-1],) and len(c.base["x"]) == c.Q
    worst = dict(influence=0.0, x=0.0, value=0.0)
    swaps = 0
    for q, ref in enumerate(c.refs):
        assert (ref["n"] == 0) == (q == EMPTY)
        swaps += check_against(c.base, q, ref, "S%d" % q, worst)
    # the 64-item slate, all coupled
    assert c.long_ref["cond"] < COND_MAX and c.long["offsets"].tolist() == [0, c.long_ref["n"]]
    swaps += check_against(c.long, 0, c.long_ref, "64 items", worst)
    print("largest rel err: influence %.2e, x %.2e, value %.2e; near-tie swaps %d" % (
        worst["influence"], worst["x"], worst["value"], swaps))


def test_two_items_are_the_pair_call(case):
    """S0 = (0; 7, 8; 1, -1) against get_pair_influence_batch's (0, 7, 8), where that call exists:
    the ratings, the gap and x block for block within RTOL (not bitwise: the elimination differs)."""
    c = case
    if (c.model, c.k) not in PAIR_SIZES:
        with pytest.raises(FIAError, match="unsupported"):
            c.m.get_pair_influence_batch([0], [c.slates[0][1]], K=K, full=True)
        return
    pr = c.m.get_pair_influence_batch([0], [c.slates[0][1]], K=K, full=True)
    assert np.array_equal(pr["rel_idx"], c.base["rel_idx"][span(c.base, 0)])
    scale = np.abs(pr["influence"]).max()
    assert np.abs(c.base["influence"][span(c.base, 0)] - pr["influence"]).max() / scale < RTOL
    assert abs(c.base["value"][0] - pr["diff"][0]) <= RTOL * abs(pr["diff"][0])
    # the same extended order at m = 2, so block for block is index for index
    for blk in slate_blocks(c.model, c.k, 2):
        assert rel_err(c.base["x"][0][blk], pr["x"][0][blk]) < RTOL


def test_one_item_is_the_single_query(case):
    """S1 (uncoupled) and S9 (n = 4) against get_influence_batch at every size, within RTOL."""
    c = case
    one = c.m.get_influence_batch([1, 2], K=K, full=True)
    for t, q in enumerate((1, 9)):
        assert len(c.slates[q]) == 1 and c.weights[q] == [1.0]
        assert np.array_equal(one["rel_idx"][span(one, t)], c.base["rel_idx"][span(c.base, q)])
        assert rel_err(c.base["influence"][span(c.base, q)], one["influence"][span(one, t)]) < RTOL
        assert rel_err(c.base["x"][q], one["x"][t]) < RTOL


def test_not_the_weighted_sum_of_singles(case):
    """S2 on user 0's list: the slate values are not the weighted sum of the six single queries'
    values on the same rows (computed on the CPU from the oracle), and the device holds the slate
    reference's.  At MF k=64 and NCF k=32 this is also the evidence that the sizes the pair call
    refuses are served."""
    from oracle import fia_oracle as fo
    c = case
    u, items, w = c.sl[2]
    du = int((c.tu == u).sum())
    ref = c.refs[2]["influence"]
    y = np.asarray(c.tr, np.float32).astype(np.float64)
    singles = sum(w[l] * fo.query(c.model, c.p, c.k, c.tu, c.ti, y, u, b, WD, DAMP)["influence"][:du]
                  for l, b in enumerate(items))
    gap = np.abs(ref[:du] - singles).max() / np.abs(ref).max()
    print("largest |slate - weighted singles| / largest |slate| on the user's list: %.3e" % gap)
    assert gap > 1e-3
    got = c.base["influence"][span(c.base, 2)][:du]
    assert np.abs(got - ref[:du]).max() / np.abs(ref).max() < RTOL
    assert np.abs(got - singles).max() / np.abs(ref).max() > 1e-3


def device_batch(c, users, slates, weights):
    import torch
    dev = c.m.ctx.torch_device
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)
    soff = np.cumsum([0] + [len(s) for s in slates])
    items = np.concatenate([np.asarray(s, np.int64) for s in slates] + [np.zeros(0, np.int64)])
    wts = np.concatenate([np.asarray(w, np.float64) for w in weights] + [np.zeros(0)])
    return t(users, np.int32), t(soff, np.int64), t(items, np.int32), t(wts, np.float64), soff


def test_bits(case):
    """Identical bits in every output: a second call; the batch reversed; S12 against S0; the top-K
    without the full vectors; each output alone through the binding; and after prepare_for on
    exactly the batch's users and items.  Ends with a full prepare."""
    import torch
    c = case
    fwd = list(range(c.Q))
    again = c.m.get_slate_influence_batch(c.users, c.slates, c.weights, K=K, full=True)
    for q in fwd:
        same_query(again, q, c.base, q)
    rev = c.m.get_slate_influence_batch(c.users[::-1], c.slates[::-1], c.weights[::-1], K=K, full=True)
    for q in fwd:
        same_query(rev, c.Q - 1 - q, c.base, q)
    assert c.sl[0] == c.sl[12]
    same_query(c.base, 12, c.base, 0)
    only = c.m.get_slate_influence_batch(c.users, c.slates, c.weights, K=K, full=False, return_x=False)
    assert "influence" not in only and "rel_idx" not in only and "x" not in only
    for q in fwd:
        same_query(only, q, c.base, q)
    # each output alone, the others NULL
    ctx, dev = c.m.ctx, c.m.ctx.torch_device
    qu, so, it, wt, soff = device_batch(c, c.users, c.slates, c.weights)
    offsets, total = ctx.count_related_slate(qu, so, it)
    assert total == c.base["offsets"][-1] and np.array_equal(offsets.cpu().numpy(), c.base["offsets"])
    Ds = c.m._host_num_params() // 2
    nx = Ds * (int(soff[-1]) + c.Q)
    xcat = np.concatenate(c.base["x"])
    assert xcat.size == nx
    rel = torch.full((total,), -7, dtype=torch.int32, device=dev)
    ctx.slate_batch(qu, so, it, wt, offsets, total, rel_idx=rel)
    assert np.array_equal(rel.cpu().numpy(), c.base["rel_idx"])
    infl = torch.full((total,), 7.0, dtype=torch.float64, device=dev)
    ctx.slate_batch(qu, so, it, wt, offsets, total, influence=infl)
    assert np.array_equal(bits(infl.cpu().numpy()), bits(c.base["influence"]))
    x = torch.full((nx,), 7.0, dtype=torch.float64, device=dev)
    ctx.slate_batch(qu, so, it, wt, offsets, total, x=x)
    assert np.array_equal(bits(x.cpu().numpy()), bits(xcat))
    value = torch.full((c.Q,), 7.0, dtype=torch.float64, device=dev)
    ctx.slate_batch(qu, so, it, wt, offsets, total, value=value)
    assert np.array_equal(bits(value.cpu().numpy()), bits(c.base["value"]))
    # the cover of exactly the batch's users and items
    eu = np.concatenate([[u] * len(s) for u, s in zip(c.users, c.slates)]).astype(np.int32)
    ctx.prepare_for(torch.from_numpy(eu).to(dev), it)
    try:
        sub = c.m.get_slate_influence_batch(c.users, c.slates, c.weights, K=K, full=True)
    finally:
        ctx.prepare()
    for q in fwd:
        same_query(sub, q, c.base, q)


def test_permuted_slate(case):
    """S2 with its items and weights permuted: the same system in another elimination order -- per
    item block and per rating within RTOL after mapping positions (not bitwise)."""
    c = case
    u, items, w = c.sl[2]
    perm = [3, 0, 5, 1, 4, 2]
    res = c.m.get_slate_influence_batch([u], [[items[l] for l in perm]], [[w[l] for l in perm]], K=K, full=True)
    m = len(items)
    du = int((c.tu == u).sum())
    lens = [int((c.ti == b).sum()) for b in items]
    start = np.concatenate([[du], du + np.cumsum(lens)])                 # list starts in the base order
    pstart = np.concatenate([[du], du + np.cumsum([lens[l] for l in perm])])
    back = np.concatenate([np.arange(du)] + [pstart[perm.index(l)] + np.arange(lens[l]) for l in range(m)]).astype(np.int64)
    base_infl = c.base["influence"][span(c.base, 2)]
    assert res["offsets"].tolist() == [0, base_infl.size] and start[-1] == base_infl.size
    assert np.array_equal(res["rel_idx"][back], c.base["rel_idx"][span(c.base, 2)])
    assert rel_err(res["influence"][back], base_infl) < RTOL
    assert abs(res["value"][0] - c.base["value"][2]) <= RTOL * abs(c.base["value"][2])
    blocks = slate_blocks(c.model, c.k, m)
    scale = np.abs(c.base["x"][2]).max()
    assert np.abs(res["x"][0][blocks[0]] - c.base["x"][2][blocks[0]]).max() / scale < RTOL
    for l in range(m):
        got = res["x"][0][blocks[1 + perm.index(l)]]
        assert np.abs(got - c.base["x"][2][blocks[1 + l]]).max() / scale < RTOL, l


def test_bad_slates_through_the_binding(case):
    """A user id out of range, an item id out of range, a repeated item, m = 0 and m = 65, given to
    the binding directly (the facade refuses them): never an index, n = 0 -- no ratings, a NaN x and
    value, empty top-K slots -- and the neighbours keep their bits.  Then the checks of the call."""
    import torch
    c = case
    ctx, dev = c.m.ctx, c.m.ctx.torch_device
    big = 2 ** 31 - 1
    good0, good3 = c.sl[0], c.sl[3]
    batch = [good0,
             (-1, [7, 8], [1.0, -1.0]), (U, [7, 8], [1.0, -1.0]), (big, [7, 8], [1.0, -1.0]),      # a bad user
             (0, [7, I], [1.0, -1.0]), (0, [-1, 8], [1.0, -1.0]), (0, [7, big], [1.0, -1.0]),      # a bad item
             good3,
             (0, [7, 8, 7], [1.0, -1.0, 0.5]),                                                     # a repeated item
             (0, [], []),                                                                          # m = 0
             (0, list(range(65)), [1.0] * 65),                                                     # m = 65
             good0]
    live = {0: 0, 7: 3, 11: 0}
    users, slates, weights = [b[0] for b in batch], [b[1] for b in batch], [b[2] for b in batch]
    Q = len(batch)
    qu, so, it, wt, soff = device_batch(c, users, slates, weights)
    offsets, _ = ctx.count_related_slate(qu, so, it, want_total=False)
    off = offsets.cpu().numpy()
    want_n = [c.refs[live[q]]["n"] if q in live else 0 for q in range(Q)]
    assert off.tolist() == np.cumsum([0] + want_n).tolist()
    total = int(off[-1])
    Ds = c.m._host_num_params() // 2
    nx = Ds * (int(soff[-1]) + Q)
    infl = torch.full((total,), 7.0, dtype=torch.float64, device=dev)
    rel = torch.full((total,), -7, dtype=torch.int32, device=dev)
    x = torch.full((nx,), 7.0, dtype=torch.float64, device=dev)
    value = torch.full((Q,), 7.0, dtype=torch.float64, device=dev)
    tp, ti = (torch.full((Q * K,), -7, dtype=torch.int64, device=dev) for _ in range(2))
    tv = torch.full((Q * K,), 7.0, dtype=torch.float64, device=dev)
    ctx.slate_batch(qu, so, it, wt, offsets, total, rel, infl, x, value, K, tp, ti, tv)
    xs = x.cpu().numpy()
    got = dict(offsets=off, rel_idx=rel.cpu().numpy().astype(np.int64), influence=infl.cpu().numpy(),
               x=[xs[Ds * (soff[q] + q):Ds * (soff[q + 1] + q + 1)] for q in range(Q)], value=value.cpu().numpy(),
               topk_pos=tp.cpu().numpy().reshape(Q, K), topk_idx=ti.cpu().numpy().reshape(Q, K),
               topk_val=tv.cpu().numpy().reshape(Q, K))
    for row in range(Q):
        if row in live:
            same_query(got, row, c.base, live[row])
            continue
        assert got["x"][row].size == Ds * (len(slates[row]) + 1) and np.isnan(got["x"][row]).all(), row
        assert np.isnan(got["value"][row]), row
        assert (got["topk_pos"][row] == -1).all() and (got["topk_idx"][row] == -1).all()
        assert np.isnan(got["topk_val"][row]).all()
    # with a total the count reports each of them
    for row in range(Q):
        one = device_batch(c, users[row:row + 1], slates[row:row + 1], weights[row:row + 1])
        if row in live:
            assert ctx.count_related_slate(one[0], one[1], one[2])[1] == want_n[row]
        else:
            with pytest.raises(FIAError, match="invalid argument"):
                ctx.count_related_slate(one[0], one[1], one[2])
    # total_rel != offsets[Q] (an oversized one) and no output at all: FIA_ERR_INVALID
    gq, gso, git, gwt, _ = device_batch(c, c.users, c.slates, c.weights)
    offsets, total = ctx.count_related_slate(gq, gso, git)
    with pytest.raises(FIAError, match="invalid argument.*total_rel"):
        ctx.slate_batch(gq, gso, git, gwt, offsets, 2 ** 31, influence=infl)
    with pytest.raises(FIAError, match="invalid argument.*no output"):
        ctx.slate_batch(gq, gso, git, gwt, offsets, total)
    # a cover without the slates' other items: the count with a total refuses the batch (FIA_ERR_STATE)
    ctx.prepare_for(gq, torch.from_numpy(np.array([s[0] for s in c.slates], np.int32)).to(dev))
    try:
        with pytest.raises(FIAError, match="bad call order"):
            ctx.count_related_slate(gq, gso, git)
    finally:
        ctx.prepare()
    same_query(c.m.get_slate_influence_batch(c.users[:2], c.slates[:2], c.weights[:2], K=K, full=True), 1, c.base, 1)


def test_large_k_is_unsupported(tmp_path):
    """MF k=128 through the facade: FIA_ERR_UNSUPPORTED, with a text that names the sizes."""
    tu, ti, tr = problem()
    m = make_model("MF", U, I, 128, (tu, ti, tr), (np.array([0], np.int32), np.array([7], np.int32)),
                   params_for("MF", 128), wd=WD, damping=DAMP, tmpdir=tmp_path)
    try:
        with pytest.raises(FIAError, match="unsupported.*MF k in \\{8, 16, 32, 64\\} and NCF k in \\{8, 16, 32\\}"):
            m.get_slate_influence_batch([0], [[7, 8]], K=1)
    finally:
        m.ctx.close()
