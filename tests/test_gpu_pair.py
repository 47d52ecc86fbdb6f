"""GPU tests of fia_count_related_pair / fia_pair_batch / get_pair_influence_batch: which ratings
put item i above item j for a user -- the influence of every rating of R_u ++ C_i ++ C_j on the gap
r-hat(u, i) - r-hat(u, j), from ONE system over (theta_u, theta_i, theta_j) --

    influence[offsets[q] + p] = x . (2 e_p g_p + wd M theta_t) / n,   x = H^-1 v

against pair_reference (tests/test_pair_cpu.py: the definition in numpy, row by row, checked there
against autograd), and for the properties of the call: it is not the difference of two single
queries, the swap of i and j, the bits (a second call, the batch reversed, outputs alone, the
prepare_for cover), bad ids through the binding and the unsupported sizes.

Tolerance: the project's RTOL = 1e-5 relative to the largest |want| of the query (rel_err).  Both
sides work in fp64; every pair is asserted (tests/test_pair_cpu.py) to give cond(H) < 1e8.

The problem is that of tests/test_newton_cpu.py (20 users x 320 items; user 0's 300 ratings cross a
256-position scoring tile; item lists of 1, 15, 16, 17 and about 10; a duplicated pair; empty
entities); the batch is pair_list's twelve pairs plus (19, 318, 319) with n = 0."""
import numpy as np
import pytest

from influence._lib import FIAError
from test_cand_newton_cpu import params_for
from test_gpu_parity import RTOL, check_topk, make_model, rel_err
from test_newton_cpu import DAMP, I, U, WD, problem
from test_pair_cpu import SIZES, pair_blocks, pair_list, pair_reference

pytestmark = pytest.mark.gpu

K = 4
EMPTY = (19, 318, 319)
OUTS = ("rel_idx", "influence", "x", "diff", "topk_pos", "topk_idx", "topk_val")


class Case(object):
    pass


@pytest.fixture(scope="module", params=SIZES, ids=lambda v: "%s-k%d" % v)
def case(request, tmp_path_factory):
    model, k = request.param
    c = Case()
    c.model, c.k = model, k
    c.tu, c.ti, c.tr = tu, ti, tr = problem()
    c.p = params_for(model, k)
    c.qs = pair_list(tu, ti) + [EMPTY]
    c.Q = len(c.qs)
    c.u = np.array([q[0] for q in c.qs], np.int32)
    c.i = np.array([q[1] for q in c.qs], np.int32)
    c.j = np.array([q[2] for q in c.qs], np.int32)
    # test rows 0 .. Q-1 are the pairs' (u, i), rows Q .. 2Q-1 their (u, j): the swapped batch
    c.m = make_model(model, U, I, k, (tu, ti, tr), (np.concatenate([c.u, c.u]), np.concatenate([c.i, c.j])), c.p,
                     wd=WD, damping=DAMP, tmpdir=tmp_path_factory.mktemp("pair_%s%d" % (model, k)))
    # the reference, once per distinct pair
    seen = {}
    for q in c.qs:
        if q not in seen:
            seen[q] = pair_reference(model, c.p, k, tu, ti, tr, q[0], q[1], q[2], WD, DAMP)
    c.refs = [seen[q] for q in c.qs]
    c.fwd = list(range(c.Q))
    c.base = c.m.get_pair_influence_batch(c.fwd, c.j, K=K, full=True)
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
    for key in ("x", "diff", "topk_val"):
        if key in a and key in b:
            assert np.array_equal(bits(a[key][qa]), bits(b[key][qb])), (key, qa, qb)
    for key in ("topk_pos", "topk_idx"):
        if key in a and key in b:
            assert np.array_equal(a[key][qa], b[key][qb]), (key, qa, qb)


def test_matches_reference(case):
    c = case
    off = c.base["offsets"]
    assert off.tolist() == np.cumsum([0] + [r["n"] for r in c.refs]).tolist()
    assert c.base["influence"].shape == (off[-1],) and c.base["x"].shape == (c.Q, c.refs[0]["x"].size)
    worst = dict(influence=0.0, x=0.0, diff=0.0)
    swaps = 0
    for q, ref in enumerate(c.refs):
        got = c.base["influence"][span(c.base, q)]
        assert np.array_equal(c.base["rel_idx"][span(c.base, q)], ref["rel"]), c.qs[q]
        pos = c.base["topk_pos"][q]
        if not ref["n"]:
            assert c.qs[q] == EMPTY and got.size == 0 and np.isnan(c.base["x"][q]).all()
            assert np.isfinite(c.base["diff"][q]) and rel_err(c.base["diff"][q:q + 1], np.array([ref["diff"]])) < RTOL
            assert (pos == -1).all() and (c.base["topk_idx"][q] == -1).all() and np.isnan(c.base["topk_val"][q]).all()
            continue
        errs = dict(influence=rel_err(got, ref["influence"]), x=rel_err(c.base["x"][q], ref["x"]),
                    diff=rel_err(c.base["diff"][q:q + 1], np.array([ref["diff"]])))
        print("pair %s n %d rel err influence %.2e x %.2e diff %.2e (cond %.2e)" % (
            c.qs[q], ref["n"], errs["influence"], errs["x"], errs["diff"], ref["cond"]))
        for key, err in errs.items():
            worst[key] = max(worst[key], err)
            assert err < RTOL, (c.qs[q], key, err)
        swaps += check_topk(pos, got, ref["influence"], K)
        m = min(K, ref["n"])
        assert np.array_equal(c.base["topk_idx"][q, :m], ref["rel"][pos[:m]])
        assert np.array_equal(bits(c.base["topk_val"][q, :m]), bits(got[pos[:m]]))
        assert (c.base["topk_idx"][q, m:] == -1).all() and np.isnan(c.base["topk_val"][q, m:]).all()
    print("largest rel err: influence %.2e, x %.2e, diff %.2e; near-tie swaps %d" % (
        worst["influence"], worst["x"], worst["diff"], swaps))


def test_not_the_difference_of_singles(case):
    """(0, 7, 8) on user 0's list: the pair values are not get_influence_batch's (0, 7) minus (0, 8)
    values on the same rows -- the gap computed on the CPU from the references -- and the device
    holds the pair reference's."""
    from oracle import fia_oracle as fo
    c = case
    u, i, j = c.qs[0]
    du = int((c.tu == u).sum())
    ref = c.refs[0]["influence"][:du]
    single = [fo.query(c.model, c.p, c.k, c.tu, c.ti, c.tr, u, b, WD, DAMP) for b in (i, j)]
    assert np.array_equal(single[0]["rel"][:du], c.refs[0]["rel"][:du])
    gap = np.abs(ref - (single[0]["influence"][:du] - single[1]["influence"][:du])).max() / np.abs(ref).max()
    print("largest |pair - (single i - single j)| / largest |pair| on the user's list: %.3e" % gap)
    assert gap > 1e-3
    got = c.base["influence"][span(c.base, 0)][:du]
    assert np.abs(got - ref).max() / np.abs(c.refs[0]["influence"]).max() < RTOL


def test_swap(case):
    """The batch with i and j swapped: every influence and the gap negated, the item blocks of x
    swapped and negated, within RTOL."""
    c = case
    sw = c.m.get_pair_influence_batch([c.Q + q for q in c.fwd], c.i, K=K, full=True)
    bu, bi, bj = pair_blocks(c.model, c.k)
    worst = 0.0
    for q, ref in enumerate(c.refs):
        du, di, dj = ((c.tu == c.qs[q][0]).sum(), (c.ti == c.qs[q][1]).sum(), (c.ti == c.qs[q][2]).sum())
        back = np.concatenate([np.arange(du), du + dj + np.arange(di), du + np.arange(dj)]).astype(np.int64)
        assert span(sw, q).stop - span(sw, q).start == ref["n"]
        assert abs(sw["diff"][q] + c.base["diff"][q]) <= RTOL * abs(c.base["diff"][q])
        if not ref["n"]:
            continue
        assert np.array_equal(sw["rel_idx"][span(sw, q)][back], ref["rel"])
        xs = np.zeros_like(ref["x"])
        xs[bu], xs[bi], xs[bj] = -sw["x"][q][bu], -sw["x"][q][bj], -sw["x"][q][bi]
        errs = (rel_err(-sw["influence"][span(sw, q)][back], c.base["influence"][span(c.base, q)]),
                rel_err(xs, c.base["x"][q]))
        worst = max(worst, *errs)
        assert max(errs) < RTOL, (c.qs[q], errs)
    print("largest rel err of the swapped batch against the negated results %.2e" % worst)


def test_bits(case):
    """Identical bits in every output: a second call; the batch reversed; the first pair again at the
    end; the top-K without the full vectors; each output alone through the binding; and after
    prepare_for on exactly the u, i and j of the batch.  Ends with a full prepare."""
    import torch
    c = case
    again = c.m.get_pair_influence_batch(c.fwd, c.j, K=K, full=True)
    for q in c.fwd:
        same_query(again, q, c.base, q)
    rev = c.m.get_pair_influence_batch(c.fwd[::-1], c.j[::-1], K=K, full=True)
    for q in c.fwd:
        same_query(rev, c.Q - 1 - q, c.base, q)
    assert c.qs[0] == c.qs[11]
    same_query(c.base, 11, c.base, 0)
    only = c.m.get_pair_influence_batch(c.fwd, c.j, K=K, full=False, return_x=False)
    assert "influence" not in only and "rel_idx" not in only and "x" not in only
    for q in c.fwd:
        same_query(only, q, c.base, q)
    # each output alone, the others NULL
    ctx, dev = c.m.ctx, c.m.ctx.torch_device
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(dev)
    qu, qi, qj = t(c.u), t(c.i), t(c.j)
    offsets, total = ctx.count_related_pair(qu, qi, qj)
    assert total == c.base["offsets"][-1] and np.array_equal(offsets.cpu().numpy(), c.base["offsets"])
    D3 = c.base["x"].shape[1]
    rel = torch.full((total,), -7, dtype=torch.int32, device=dev)
    ctx.pair_batch(qu, qi, qj, offsets, total, rel_idx=rel)
    assert np.array_equal(rel.cpu().numpy(), c.base["rel_idx"])
    infl = torch.full((total,), 7.0, dtype=torch.float64, device=dev)
    ctx.pair_batch(qu, qi, qj, offsets, total, influence=infl)
    assert np.array_equal(bits(infl.cpu().numpy()), bits(c.base["influence"]))
    x = torch.full((c.Q * D3,), 7.0, dtype=torch.float64, device=dev)
    ctx.pair_batch(qu, qi, qj, offsets, total, x=x)
    assert np.array_equal(bits(x.cpu().numpy().reshape(c.Q, D3)), bits(c.base["x"]))
    diff = torch.full((c.Q,), 7.0, dtype=torch.float64, device=dev)
    ctx.pair_batch(qu, qi, qj, offsets, total, diff=diff)
    assert np.array_equal(bits(diff.cpu().numpy()), bits(c.base["diff"]))
    # the cover of exactly the batch's u, i and j
    c.m.prepare_for(c.fwd, other_items=c.j)
    try:
        sub = c.m.get_pair_influence_batch(c.fwd, c.j, K=K, full=True)
    finally:
        c.m.ctx.prepare()
    for q in c.fwd:
        same_query(sub, q, c.base, q)


def test_bad_queries_through_the_binding(case):
    """Ids out of range (-1, U, 2^31 - 1) and i == j, given to the binding directly (the facade
    refuses them): never an index, n = 0 -- no ratings, a NaN x, empty top-K slots; diff NaN for a
    bad id and +0.0 for i == j -- and the neighbours keep their bits.  Then the checks of the call."""
    import torch
    c = case
    ctx, dev = c.m.ctx, c.m.ctx.torch_device
    t = lambda a, dt=np.int32: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)
    big = 2 ** 31 - 1
    (u0, i0, j0), (u1, i1, j1) = c.qs[0], c.qs[2]
    us = [u0, -1, U, u0, u1, u0, big, u0]
    iis = [i0, i0, i0, I, i1, i0, i0, big]
    js = [j0, j0, j0, j0, j1, i0, j0, j0]
    live = {0: 0, 4: 2}
    qu, qi, qj = t(us), t(iis), t(js)
    Q = len(us)
    offsets, _ = ctx.count_related_pair(qu, qi, qj, want_total=False)
    off = offsets.cpu().numpy()
    n0, n1 = c.refs[0]["n"], c.refs[2]["n"]
    assert off.tolist() == [0, n0, n0, n0, n0, n0 + n1, n0 + n1, n0 + n1, n0 + n1]
    total = int(off[-1])
    D3 = c.base["x"].shape[1]
    infl = torch.full((total,), 7.0, dtype=torch.float64, device=dev)
    rel = torch.full((total,), -7, dtype=torch.int32, device=dev)
    x = torch.full((Q * D3,), 7.0, dtype=torch.float64, device=dev)
    diff = torch.full((Q,), 7.0, dtype=torch.float64, device=dev)
    tp, ti = (torch.full((Q * K,), -7, dtype=torch.int64, device=dev) for _ in range(2))
    tv = torch.full((Q * K,), 7.0, dtype=torch.float64, device=dev)
    ctx.pair_batch(qu, qi, qj, offsets, total, rel, infl, x, diff, K, tp, ti, tv)
    got = dict(offsets=off, rel_idx=rel.cpu().numpy().astype(np.int64), influence=infl.cpu().numpy(),
               x=x.cpu().numpy().reshape(Q, D3), diff=diff.cpu().numpy(), topk_pos=tp.cpu().numpy().reshape(Q, K),
               topk_idx=ti.cpu().numpy().reshape(Q, K), topk_val=tv.cpu().numpy().reshape(Q, K))
    for row in range(Q):
        if row in live:
            same_query(got, row, c.base, live[row])
            continue
        assert np.isnan(got["x"][row]).all()
        assert (got["topk_pos"][row] == -1).all() and (got["topk_idx"][row] == -1).all()
        assert np.isnan(got["topk_val"][row]).all()
        if row == 5:                                    # i == j
            assert bits(got["diff"][row:row + 1])[0] == 0
        else:
            assert np.isnan(got["diff"][row])
    # with a total the count reports the bad ids
    with pytest.raises(FIAError, match="invalid argument"):
        ctx.count_related_pair(qu, qi, qj)
    # an oversized total_rel and no output at all: FIA_ERR_INVALID
    good = (t(c.u), t(c.i), t(c.j))
    offsets, total = ctx.count_related_pair(*good)
    with pytest.raises(FIAError, match="invalid argument.*total_rel"):
        ctx.pair_batch(*good, offsets, 2 ** 31, influence=infl)
    with pytest.raises(FIAError, match="invalid argument.*no output"):
        ctx.pair_batch(*good, offsets, total)
    # a cover without the j's: the count with a total refuses the batch (FIA_ERR_STATE)
    c.m.prepare_for(c.fwd)
    try:
        with pytest.raises(FIAError, match="bad call order"):
            ctx.count_related_pair(*good)
    finally:
        ctx.prepare()
    same_query(c.m.get_pair_influence_batch(c.fwd[:2], c.j[:2], K=K, full=True), 1, c.base, 1)


@pytest.mark.parametrize("model,k", [("MF", 64), ("NCF", 32), ("MF", 128)])
def test_other_sizes_are_unsupported(model, k, tmp_path):
    """MF k=64, NCF k=32 and the large-k models: FIA_ERR_UNSUPPORTED through the facade."""
    tu, ti, tr = problem()
    qs = pair_list(tu, ti)[:2]
    qu = np.array([q[0] for q in qs], np.int32)
    qi = np.array([q[1] for q in qs], np.int32)
    m = make_model(model, U, I, k, (tu, ti, tr), (qu, qi), params_for(model, k), wd=WD, damping=DAMP, tmpdir=tmp_path)
    try:
        with pytest.raises(FIAError, match="unsupported.*MF k in \\{8, 16, 32\\} and NCF k in \\{8, 16\\}"):
            m.get_pair_influence_batch([0, 1], [q[2] for q in qs], K=1)
    finally:
        m.ctx.close()
