"""GPU tests of fia_query_batch_newton / get_newton_influence_batch: the Newton-corrected influence
of EVERY related rating of a test prediction,

    newton[offsets[q] + p] = v . (H - H_{j})^-1 b_{j},   j = rel[p]

against newton_reference (tests/test_newton_cpu.py: fia_group_influence's definition for the
singleton group of every related position, restated in numpy from the fp64 oracle), and for the
properties of the call: own-pair positions, the difference to first order, top-K, determinism,
the prepare_for cover, the query chunking and the unsupported sizes.

Tolerance: the project's RTOL = 1e-5 relative to the largest |want| of the query (rel_err).  Both
sides work in fp64; every tested position is asserted (on the CPU) to leave a system with
cond(H - H_j) < 1e8.

The problem and the queries are those of tests/test_newton_cpu.py (20 users x 320 items; user 0's
300 ratings cross a 256-rating chunk and leave a tile tail of 12; item lists of 1, 15, 16, 17
and about 10; a duplicated pair; empty entities)."""
import os

import numpy as np
import pytest

from influence import synth
from influence._lib import FIAError
from test_group_cpu import w3g_of
from test_gpu_parity import RTOL, make_model, rel_err
from test_newton_cpu import DAMP, DUP, I, U, WD, newton_reference, problem, queries

pytestmark = pytest.mark.gpu

SIZES = [("MF", 8), ("MF", 16), ("MF", 32), ("MF", 64), ("NCF", 8), ("NCF", 16), ("NCF", 32)]
COND_MAX = 1e8


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
    c.Q = len(c.qs)
    qu = np.array([q[0] for q in c.qs], np.int32)
    qi = np.array([q[1] for q in c.qs], np.int32)
    c.m = make_model(model, U, I, k, (tu, ti, tr), (qu, qi), c.p, wd=WD, damping=DAMP,
                     tmpdir=tmp_path_factory.mktemp("newton_%s%d" % (model, k)))
    W3g = w3g_of(model, c.p, k)
    # the reference, once per distinct pair
    c.cores, c.refs, seen = [], [], {}
    for (u, i) in c.qs:
        if (u, i) not in seen:
            core = fo.query(model, c.p, k, tu, ti, tr, u, i, WD, DAMP)
            seen[(u, i)] = (core, newton_reference(core, WD, DAMP, W3g) if core["n"] else None)
        c.cores.append(seen[(u, i)][0])
        c.refs.append(seen[(u, i)][1])
    c.live = [q for q in range(c.Q) if c.cores[q]["n"]]
    c.base = c.m.get_newton_influence_batch(list(range(c.Q)), K=4, full=True)
    yield c
    c.m.ctx.close()


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def span(c, q, res=None):
    off = (res or c.base)["offsets"]
    return slice(int(off[q]), int(off[q + 1]))


def test_matches_reference(case):
    """Every position of every live query against the per-position singleton solve; the train
    rows are get_influence_batch's."""
    c = case
    off = c.base["offsets"]
    assert off.tolist() == np.cumsum([0] + [c.cores[q]["n"] for q in range(c.Q)]).tolist()
    assert c.base["newton"].shape == (off[-1],)
    worst, worst_cond = 0.0, 0.0
    for q in c.live:
        ref = c.refs[q]
        assert ref["cond"].max() < COND_MAX, (c.qs[q], ref["cond"].max())
        worst_cond = max(worst_cond, ref["cond"].max())
        got = c.base["newton"][span(c, q)]
        assert np.isfinite(got).all()
        err = rel_err(got, ref["newton"])
        print("query %s n %d rel err %.2e (largest |want| %.3e, smallest |1 - c h| %.1e)" % (
            c.qs[q], c.cores[q]["n"], err, np.abs(ref["newton"]).max(), ref["min_den"]))
        worst = max(worst, err)
        assert err < RTOL, (c.qs[q], err)
        assert np.array_equal(c.base["rel_idx"][span(c, q)], c.cores[q]["rel"])
    print("largest rel err %.2e, largest cond(H - H_j) %.3e" % (worst, worst_cond))
    first = c.m.get_influence_batch(list(range(c.Q)), K=0, full=True, return_x=False)
    assert np.array_equal(first["offsets"], off) and np.array_equal(first["rel_idx"], c.base["rel_idx"])


def test_own_pair_positions(case):
    """Both positions of an own-pair row hold the same bits; the two rows of the duplicated pair
    (different ratings) differ."""
    c = case
    seen = 0
    for q in c.live:
        rel, own = c.cores[q]["rel"], c.refs[q]["own"]
        got = c.base["newton"][span(c, q)]
        for r in np.unique(rel[own]):
            a, b = np.nonzero(rel == r)[0]
            assert bits(got[a:a + 1])[0] == bits(got[b:b + 1])[0], (c.qs[q], r)
            seen += 1
    assert seen == 1 + 2 + 1                            # (0, i0) twice in the batch, the duplicated pair's two rows
    q = c.qs.index(DUP)
    rows = np.unique(c.cores[q]["rel"][c.refs[q]["own"]])
    got = c.base["newton"][span(c, q)]
    va, vb = (got[np.nonzero(c.cores[q]["rel"] == r)[0][0]] for r in rows)
    assert rows.size == 2 and va != vb


def test_corrected_differs_from_first_order_and_is_the_singleton_group(case):
    """User 0's train-row query: the corrected value is not the first-order one, and it is
    get_group_influence of the singleton group, for 20 positions with the own-pair row among them."""
    c = case
    first = c.m.get_influence_batch(list(range(c.Q)), K=0, full=True, return_x=False)
    got, infl = c.base["newton"][span(c, 0)], first["influence"][span(c, 0)]
    diff = np.abs(got - infl).max() / np.abs(infl).max()
    print("largest |newton - first order| / largest |first order| %.3e" % diff)
    assert diff > 100 * RTOL
    rel, own = c.cores[0]["rel"], c.refs[0]["own"]
    rng = np.random.default_rng(5)
    pos = np.concatenate([np.nonzero(own)[0][:1], rng.choice(np.nonzero(~own)[0], 19, replace=False)])
    groups = [[np.array([rel[p]]) for p in pos]] + [[] for _ in range(c.Q - 1)]
    grp = c.m.get_group_influence(list(range(c.Q)), groups)["group"]
    assert grp.shape == (20,)
    err = np.abs(grp - got[pos]).max() / np.abs(grp).max()
    print("rel err against singleton groups %.2e" % err)
    assert err < RTOL


@pytest.mark.parametrize("K", [1, 4, 64])
def test_topk(case, K):
    """The top-K is a stable argsort of |newton| from the full output; slots past n_q hold -1 / NaN;
    without the full vectors the same bits."""
    c = case
    res = c.base if K == 4 else c.m.get_newton_influence_batch(list(range(c.Q)), K=K, full=True)
    only = c.m.get_newton_influence_batch(list(range(c.Q)), K=K, full=False)
    assert "newton" not in only and np.array_equal(only["offsets"], res["offsets"])
    assert np.array_equal(bits(res["newton"]), bits(c.base["newton"]))
    for key in ("topk_pos", "topk_idx"):
        assert res[key].shape == (c.Q, K) and np.array_equal(res[key], only[key]), key
    assert np.array_equal(bits(res["topk_val"]), bits(only["topk_val"]))
    for q in range(c.Q):
        vals = res["newton"][span(c, q, res)]
        n = vals.size
        order = np.argsort(-np.abs(vals), kind="stable")[:K]
        m = order.size
        assert np.array_equal(res["topk_pos"][q, :m], order), (q, K)
        assert np.array_equal(bits(res["topk_val"][q, :m]), bits(vals[order]))
        assert np.array_equal(res["topk_idx"][q, :m], res["rel_idx"][span(c, q, res)][order])
        assert (res["topk_pos"][q, m:] == -1).all() and (res["topk_idx"][q, m:] == -1).all()
        assert np.isnan(res["topk_val"][q, m:]).all()
        assert m == min(n, K)


def test_reproducible_and_position_independent(case):
    """A second call gives the same bits; the first pair again at the end of the batch gives the
    bits of the first; the n_q = 0 query wrote nothing."""
    c = case
    again = c.m.get_newton_influence_batch(list(range(c.Q)), K=4, full=True)
    for key in ("newton", "topk_val"):
        assert np.array_equal(bits(again[key]), bits(c.base[key])), key
    assert np.array_equal(again["topk_pos"], c.base["topk_pos"])
    assert c.qs[0] == c.qs[-1]
    assert np.array_equal(bits(c.base["newton"][span(c, 0)]), bits(c.base["newton"][span(c, c.Q - 1)]))
    assert np.array_equal(bits(c.base["topk_val"][0]), bits(c.base["topk_val"][-1]))
    empty = [q for q in range(c.Q) if not c.cores[q]["n"]]
    assert len(empty) == 1 and span(c, empty[0]).start == span(c, empty[0]).stop
    assert (c.base["topk_pos"][empty[0]] == -1).all() and np.isnan(c.base["topk_val"][empty[0]]).all()


def test_query_chunks_give_the_bits_of_one_launch(case):
    """The queries-per-launch limit lowered through the testing knob (FIA_NEWTON_CHUNK), so the
    batch runs in several launches."""
    c = case
    assert c.Q > 2 * 5
    os.environ["FIA_NEWTON_CHUNK"] = "5"
    try:
        chunked = c.m.get_newton_influence_batch(list(range(c.Q)), K=4, full=True)
        only = c.m.get_newton_influence_batch(list(range(c.Q)), K=4, full=False)
    finally:
        del os.environ["FIA_NEWTON_CHUNK"]
    for key in ("newton", "topk_val"):
        assert np.array_equal(bits(chunked[key]), bits(c.base[key])), key
    for key in ("rel_idx", "topk_pos", "topk_idx"):
        assert np.array_equal(chunked[key], c.base[key]), key
    assert np.array_equal(bits(only["topk_val"]), bits(c.base["topk_val"]))
    assert np.array_equal(only["topk_pos"], c.base["topk_pos"])


def test_out_of_range_ids_through_the_binding(case):
    """A query id outside [0, num_users) x [0, num_items), given to Context.query_batch_newton
    directly (the facade's count would refuse it): never an index, n_q = 0 -- nothing written, empty
    top-K slots -- and its neighbours keep their bits."""
    import torch
    c = case
    ctx = c.m.ctx
    dev = ctx.torch_device
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)
    (u0, i0), (u1, i1) = c.qs[0], c.qs[1]
    qu, qi = t([u0, U, -1, u1, u1], np.int32), t([i0, i0, i0, i1, I], np.int32)
    offsets, _ = ctx.count_related(qu, qi, want_total=False)
    off = offsets.cpu().numpy()
    total = int(off[-1])
    n0, n1 = c.cores[0]["n"], c.cores[1]["n"]
    assert off.tolist() == [0, n0, n0, n0, n0 + n1, n0 + n1]
    K = 4
    nw = torch.full((total,), 7.0, dtype=torch.float64, device=dev)
    rel = torch.full((total,), -7, dtype=torch.int32, device=dev)
    tp, ti = (torch.full((5 * K,), -7, dtype=torch.int64, device=dev) for _ in range(2))
    tv = torch.full((5 * K,), 7.0, dtype=torch.float64, device=dev)
    ctx.query_batch_newton(qu, qi, offsets, total, rel, nw, K, tp, ti, tv)
    nw, tp, tv = nw.cpu().numpy(), tp.cpu().numpy().reshape(5, K), tv.cpu().numpy().reshape(5, K)
    want = np.concatenate([c.base["newton"][span(c, 0)], c.base["newton"][span(c, 1)]])
    assert np.array_equal(bits(nw), bits(want))
    for row, q in ((0, 0), (3, 1)):
        assert np.array_equal(tp[row], c.base["topk_pos"][q]) and np.array_equal(bits(tv[row]), bits(c.base["topk_val"][q]))
    for row in (1, 2, 4):
        assert (tp[row] == -1).all() and np.isnan(tv[row]).all()


def test_cover_independent(case):
    """After prepare_for on the batch, the results are bitwise those after the full prepare.  Runs
    last on the model."""
    c = case
    c.m.prepare_for(c.live)
    try:
        sub = c.m.get_newton_influence_batch(c.live, K=4, full=True)
    finally:
        c.m.ctx.prepare()
    want = np.concatenate([c.base["newton"][span(c, q)] for q in c.live])
    assert np.array_equal(bits(sub["newton"]), bits(want))
    assert np.array_equal(bits(sub["topk_val"]), bits(c.base["topk_val"][c.live]))
    assert np.array_equal(sub["topk_pos"], c.base["topk_pos"][c.live])


def test_large_k_is_unsupported(tmp_path):
    """The large-k models are the follow-up: FIA_ERR_UNSUPPORTED through the facade, with a text
    that says so."""
    tu, ti, tr = problem()
    qs = queries(tu, ti)[:2]
    qu = np.array([q[0] for q in qs], np.int32)
    qi = np.array([q[1] for q in qs], np.int32)
    m = make_model("MF", U, I, 128, (tu, ti, tr), (qu, qi), synth.mf_params(U, I, 128, 3), wd=WD, damping=DAMP,
                   tmpdir=tmp_path)
    try:
        with pytest.raises(FIAError, match="unsupported.*large-k"):
            m.get_newton_influence_batch([0, 1], K=1)
    finally:
        m.ctx.close()
