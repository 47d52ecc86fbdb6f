"""GPU tests of fia_score_candidates_newton / get_candidate_newton_batch: the Newton-corrected
influence of hypothetical ratings,

    newton_add[c] = v . (H + H_c)^-1 b_c

against cand_newton_reference (tests/test_cand_newton_cpu.py: the definition in numpy, one solve per
candidate, from the fp64 oracle), and for the properties of the call: the candidates sharing neither
side, the difference to first order, top-K, reproducibility under every rearrangement of the batch,
the prepare_for cover, the argument checks and the unsupported sizes.

Tolerance: the project's RTOL = 1e-5 relative to the largest |want| of the query (rel_err).  Both
sides work in fp64; every candidate is asserted (on the CPU) to give cond(H + H_c) < 1e8.

The problem and the queries are those of tests/test_newton_cpu.py; the candidate lists are
candidate_lists of tests/test_cand_newton_cpu.py (a 300-candidate user-side segment that crosses a
256-position tile and leaves a tail of 12, the two sides interleaved, segments of 1, 15, 16, 17, 64
and 65, an empty list, `both` candidates at a train row, the duplicated pair and a non-train pair,
bad ids, an n_q = 0 query, and one candidate listed twice 300 positions apart).  The batch goes
through Context.score_candidates_newton: the facade refuses the bad ids on the host."""
import os

import numpy as np
import pytest

from influence import synth
from influence._lib import FIAError
from test_cand_newton_cpu import (COND_MAX, SIZES, cand_newton_reference, candidate_gradients, candidate_lists,
                                  params_for)
from test_group_cpu import w3g_of
from test_gpu_parity import RTOL, make_model, rel_err
from test_newton_cpu import DAMP, I, U, WD, problem, queries

pytestmark = pytest.mark.gpu


class Case(object):
    pass


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def run(c, qs, off, cu, ci, cy, K=0, full=True):
    """One call through the binding: (newton_add or None, topk_pos [Q, K] or None, topk_val)."""
    import torch
    ctx = c.m.ctx
    dev = ctx.torch_device
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)
    Q, m = len(qs), int(off[-1])
    qu, qi = t([q[0] for q in qs], np.int32), t([q[1] for q in qs], np.int32)
    nw = torch.full((max(m, 1),), 7.0, dtype=torch.float64, device=dev) if full else None
    tp = torch.full((Q * K,), -7, dtype=torch.int64, device=dev) if K else None
    tv = torch.full((Q * K,), 7.0, dtype=torch.float64, device=dev) if K else None
    ctx.score_candidates_newton(qu, qi, t(off, np.int64), m, t(cu, np.int32), t(ci, np.int32), t(cy, np.float32), nw,
                                K, tp, tv)
    return (nw[:m].cpu().numpy() if full else None, tp.cpu().numpy().reshape(Q, K) if K else None,
            tv.cpu().numpy().reshape(Q, K) if K else None)


@pytest.fixture(scope="module", params=SIZES, ids=lambda v: "%s-k%d" % v)
def case(request, tmp_path_factory):
    from oracle import fia_oracle as fo
    model, k = request.param
    c = Case()
    c.model, c.k = model, k
    c.tu, c.ti, c.tr = tu, ti, tr = problem()
    c.p = params_for(model, k)
    c.qs = queries(tu, ti)
    c.Q = len(c.qs)
    c.off, c.cu, c.ci, c.cy, c.dup = candidate_lists(tu, ti, c.qs)
    qu = np.array([q[0] for q in c.qs], np.int32)
    qi = np.array([q[1] for q in c.qs], np.int32)
    c.m = make_model(model, U, I, k, (tu, ti, tr), (qu, qi), c.p, wd=WD, damping=DAMP,
                     tmpdir=tmp_path_factory.mktemp("cand_newton_%s%d" % (model, k)))
    W3g = w3g_of(model, c.p, k)
    # the reference, once: NaN exactly at the bad ids and at the n_q = 0 query
    c.valid = (c.cu >= 0) & (c.cu < U) & (c.ci >= 0) & (c.ci < I)
    c.want = np.full(c.cu.size, np.nan)
    c.first = np.full(c.cu.size, np.nan)
    c.neither = np.zeros(c.cu.size, bool)
    c.cpp = np.full(c.Q, np.nan)
    c.cond, cores = 0.0, {}
    for q, (u, i) in enumerate(c.qs):
        if (u, i) not in cores:
            cores[(u, i)] = fo.query(model, c.p, k, tu, ti, tr, u, i, WD, DAMP)
        core = cores[(u, i)]
        sl = np.arange(c.off[q], c.off[q + 1])
        sl = sl[c.valid[sl]]
        if not core["n"] or not sl.size:
            continue
        G, e, both = candidate_gradients(model, c.p, k, u, i, c.cu[sl], c.ci[sl], c.cy[sl])
        ref = cand_newton_reference(core, G, e, both, WD, W3g)
        c.want[sl], c.first[sl], c.cpp[q] = ref["newton"], ref["first"], ref["cpp"]
        c.neither[sl] = (c.cu[sl] != u) & (c.ci[sl] != i)
        c.cond = max(c.cond, ref["cond"].max())
    c.base, c.base_pos, c.base_val = run(c, c.qs, c.off, c.cu, c.ci, c.cy, K=4)
    yield c
    c.m.ctx.close()


def span(c, q):
    return slice(int(c.off[q]), int(c.off[q + 1]))


def test_matches_reference(case):
    """Every candidate of every query against the per-candidate solve, none excluded; NaN exactly at
    the bad ids and at the n_q = 0 query."""
    c = case
    assert c.cond < COND_MAX, c.cond
    assert c.base.shape == (c.off[-1],)
    nan = np.isnan(c.want)
    expect_nan = ~c.valid
    expect_nan[span(c, 5)] = True
    assert np.array_equal(nan, expect_nan) and nan.sum() == 2 + 4
    assert np.array_equal(np.isnan(c.base), nan)
    worst = 0.0
    for q in range(c.Q):
        got, want = c.base[span(c, q)], c.want[span(c, q)]
        ok = ~np.isnan(want)
        if not ok.any():
            continue
        err = rel_err(got[ok], want[ok])
        print("query %s: %d candidates, rel err %.2e (largest |want| %.3e)" % (
            c.qs[q], ok.sum(), err, np.abs(want[ok]).max()))
        worst = max(worst, err)
        assert err < RTOL, (c.qs[q], err)
    print("largest rel err %.2e, largest cond(H + H_c) %.3e" % (worst, c.cond))


def test_neither_side_is_the_constant_and_first_order_differs(case):
    """A candidate sharing neither side scores c" of the reference, all of a query's with the same
    bits; and on user 0's train-row query the corrected value is not the first-order one --
    asserted on the reference, then on the device against get_candidate_influence_batch."""
    c = case
    seen = 0
    for q in range(c.Q):
        sl = np.arange(c.off[q], c.off[q + 1])
        sl = sl[c.neither[sl]]
        if not sl.size or np.isnan(c.cpp[q]):
            continue
        scale = np.abs(c.want[span(c, q)][~np.isnan(c.want[span(c, q)])]).max()
        assert np.abs(c.base[sl] - c.cpp[q]).max() < RTOL * scale, c.qs[q]
        assert (bits(c.base[sl]) == bits(c.base[sl[:1]])[0]).all(), c.qs[q]
        seen += sl.size
    assert seen >= 3 + 2
    ok = np.arange(c.off[0], c.off[1])
    ok = ok[c.valid[ok]]
    ref_diff = np.abs(c.want[ok] - c.first[ok]).max() / np.abs(c.first[ok]).max()
    assert ref_diff > 100 * RTOL, ref_diff
    X = np.stack([c.cu[ok], c.ci[ok]], 1)
    first = c.m.get_candidate_influence_batch([0], np.array([0, ok.size], np.int64), X, c.cy[ok])["influence"]
    assert rel_err(first, c.first[ok]) < RTOL
    diff = np.abs(c.base[ok] - first).max() / np.abs(first).max()
    print("largest |newton_add - first order| / largest |first order|: %.3e (reference %.3e)" % (diff, ref_diff))
    assert diff > 100 * RTOL


def check_topk(pos, val, full, K):
    """|value| descending, position ascending, NaN last; -1 / NaN in unused slots; the bits of the
    full values."""
    key = np.where(np.isnan(full), -1.0, np.abs(full))
    order = np.argsort(-key, kind="stable")[:K]
    m = order.size
    assert np.array_equal(pos[:m], order)
    assert np.array_equal(bits(val[:m]), bits(full[order]))
    assert (pos[m:] == -1).all() and np.isnan(val[m:]).all()


@pytest.mark.parametrize("K", [1, 4, 64])
def test_topk(case, K):
    c = case
    if K == 4:
        full, pos, val = c.base, c.base_pos, c.base_val
    else:
        full, pos, val = run(c, c.qs, c.off, c.cu, c.ci, c.cy, K=K)
    assert np.array_equal(bits(full), bits(c.base))
    _, opos, oval = run(c, c.qs, c.off, c.cu, c.ci, c.cy, K=K, full=False)      # top-K only
    assert np.array_equal(opos, pos) and np.array_equal(bits(oval), bits(val))
    assert pos.shape == (c.Q, K) and pos.dtype == np.int64
    for q in range(c.Q):
        check_topk(pos[q], val[q], full[span(c, q)], K)
    assert (pos[7] == -1).all()                         # the empty list
    assert np.array_equal(pos[5][:min(K, 4)], np.arange(min(K, 4)))     # n_q = 0: all NaN, in order


def test_reproducible_under_rearrangement(case):
    """A rerun, the duplicate, the queries permuted, one list permuted and five queries per launch
    all give the same bits per candidate."""
    c = case
    again, apos, aval = run(c, c.qs, c.off, c.cu, c.ci, c.cy, K=4)
    assert np.array_equal(bits(again), bits(c.base))
    assert np.array_equal(apos, c.base_pos) and np.array_equal(bits(aval), bits(c.base_val))
    a, b = c.dup
    assert b - a >= 300 and bits(c.base[a:a + 1])[0] == bits(c.base[b:b + 1])[0] and np.isfinite(c.base[a])
    rng = np.random.default_rng(9)
    # queries permuted, each with its list
    perm = rng.permutation(c.Q)
    lens = np.diff(c.off)
    poff = np.concatenate([[0], np.cumsum(lens[perm])]).astype(np.int64)
    take = np.concatenate([np.arange(c.off[q], c.off[q + 1]) for q in perm]).astype(np.int64)
    got, _, _ = run(c, [c.qs[q] for q in perm], poff, c.cu[take], c.ci[take], c.cy[take])
    assert np.array_equal(bits(got), bits(c.base[take]))
    # query 0's list permuted
    take = np.arange(c.off[-1])
    take[:c.off[1]] = rng.permutation(int(c.off[1]))
    got, _, _ = run(c, c.qs, c.off, c.cu[take], c.ci[take], c.cy[take])
    assert np.array_equal(bits(got), bits(c.base[take]))
    # several launches
    assert c.Q > 2 * 5
    os.environ["FIA_NEWTON_CHUNK"] = "5"
    try:
        chunked, cpos, cval = run(c, c.qs, c.off, c.cu, c.ci, c.cy, K=4)
        _, opos, oval = run(c, c.qs, c.off, c.cu, c.ci, c.cy, K=4, full=False)
    finally:
        del os.environ["FIA_NEWTON_CHUNK"]
    assert np.array_equal(bits(chunked), bits(c.base))
    assert np.array_equal(cpos, c.base_pos) and np.array_equal(bits(cval), bits(c.base_val))
    assert np.array_equal(opos, c.base_pos) and np.array_equal(bits(oval), bits(c.base_val))


def test_argument_checks_through_the_binding(case):
    """total_cand above FIA_CAND_MAX_TOTAL, K > 0 with null top-K arrays and no output requested:
    FIA_ERR_INVALID before anything is reserved or launched (the arrays passed are never read);
    no queries: FIA_OK."""
    import torch
    ctx = case.m.ctx
    dev = ctx.torch_device
    q = torch.zeros(1, dtype=torch.int32, device=dev)
    off = torch.zeros(2, dtype=torch.int64, device=dev)
    f = torch.zeros(1, dtype=torch.float32, device=dev)
    d = torch.zeros(1, dtype=torch.float64, device=dev)
    ptr = lambda t: t.data_ptr()
    fn = ctx.lib.fia_score_candidates_newton
    assert fn(ctx.h, 1, ptr(q), ptr(q), ptr(off), 2 ** 31, ptr(q), ptr(q), ptr(f), ptr(d), 0, None, None, None) == 1
    assert fn(ctx.h, 1, ptr(q), ptr(q), ptr(off), 0, None, None, None, ptr(d), 4, None, None, None) == 1
    assert fn(ctx.h, 1, ptr(q), ptr(q), ptr(off), 0, None, None, None, None, 0, None, None, None) == 1
    assert fn(ctx.h, 0, None, None, None, 0, None, None, None, ptr(d), 0, None, None, None) == 0


def test_facade_matches_the_binding(case):
    """get_candidate_newton_batch on the in-range candidates of three queries: the binding's bits."""
    c = case
    qsel = [0, 4, 7, 10]
    keep = np.concatenate([np.arange(c.off[q], c.off[q + 1])[c.valid[span(c, q)]] for q in qsel]).astype(np.int64)
    off = np.concatenate([[0], np.cumsum([int(c.valid[span(c, q)].sum()) for q in qsel])]).astype(np.int64)
    res = c.m.get_candidate_newton_batch(qsel, off, np.stack([c.cu[keep], c.ci[keep]], 1), c.cy[keep], K=3)
    assert np.array_equal(res["cand_offsets"], off)
    assert np.array_equal(bits(res["newton"]), bits(c.base[keep]))
    for j in range(len(qsel)):
        check_topk(res["topk_pos"][j], res["topk_val"][j], res["newton"][off[j]:off[j + 1]], 3)
    lean = c.m.get_candidate_newton_batch(qsel, off, np.stack([c.cu[keep], c.ci[keep]], 1), c.cy[keep], K=3, full=False)
    assert "newton" not in lean and np.array_equal(lean["topk_pos"], res["topk_pos"])
    assert np.array_equal(bits(lean["topk_val"]), bits(res["topk_val"]))


def test_cover_independent(case):
    """After prepare_for on the queries alone -- the candidates' entities mostly outside it -- the
    results are bitwise those after the full prepare.  Runs last on the model."""
    c = case
    live = [q for q in range(c.Q) if q != 5]
    c.m.prepare_for(live)
    try:
        sub, spos, sval = run(c, c.qs, c.off, c.cu, c.ci, c.cy, K=4)
    finally:
        c.m.ctx.prepare()
    assert np.array_equal(bits(sub), bits(c.base))
    assert np.array_equal(spos, c.base_pos) and np.array_equal(bits(sval), bits(c.base_val))


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
            m.get_candidate_newton_batch([0, 1], np.array([0, 1, 2]), np.array([[0, 1], [3, 2]]), np.array([2.5, 3.5]),
                                         K=1)
    finally:
        m.ctx.close()
