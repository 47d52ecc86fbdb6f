"""GPU tests of fia_pair_flip / get_flip_sets / get_counterfactual_explanation: the greedy
first-order set of a user's own ratings that puts item j above item i, and the re-solved system's
answer for that set,

    S = eligible rows of R_u by (val, position), taken while |S| < max_set and diff + margin + sum >= 0
    dtheta = (H - H_S)^-1 b_S,   newton = v . dtheta,   first_order = sum_S val

against flip_reference (tests/test_flip_cpu.py: the definition in numpy on pair_reference, one
stable sort and one np.linalg.solve per set), and for the properties of the call: the values are
fia_pair_batch's, first order and the re-solved system disagree where the reference says so, the
bits (a second call, the batch reversed, a query repeated, outputs alone, max_set 64 against 17, the
prepare_for cover), bad queries and argument checks through the binding, the facade and the
unsupported sizes.

Tolerance: the project's RTOL = 1e-5 relative to the largest |want| of the query (rel_err).  Both
sides work in fp64; for every case compared here tests/test_flip_cpu.py asserts cond(H - H_S) < 1e8,
sorted values further apart than 1e-7 of the largest and stopping tests further than 1e-7 from zero,
so the sets themselves are compared exactly.

The problem is that of tests/test_newton_cpu.py (user 0's 300 ratings cross a 256-position scoring
tile; user 3 holds a duplicated pair; user 17 has one rating, user 19 none); the batch is flip_batch's
cases at max_set = 64 and the first sized case again at the end."""
import numpy as np
import pytest

from influence._lib import FIA_FLIP_MAX_SET, FIAError
from test_cand_newton_cpu import params_for
from test_flip_cpu import CF_MARGIN, MAX_SET, flip_batch
from test_gpu_parity import RTOL, make_model, rel_err
from test_newton_cpu import DAMP, I, U, WD, problem
from test_pair_cpu import SIZES, pair_list

pytestmark = pytest.mark.gpu

OUTS = ("set_size", "set_row", "set_val", "first_order", "newton", "dtheta", "diff")


class Case(object):
    pass


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def call(ctx, u, i, j, margin, max_set, outs=OUTS, D3=None):
    """fia_pair_flip through the binding with the outputs named in `outs` (the others NULL), every
    buffer pre-filled with a marker; numpy arrays, the per-slot ones [Q, max_set]."""
    import torch
    dev = ctx.torch_device
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)
    Q = len(u)
    D3 = D3 or 3 * ctx.num_params() // 2
    shapes = dict(set_size=(Q, torch.int32), set_row=(Q * max_set, torch.int32), set_val=(Q * max_set, torch.float64),
                  first_order=(Q, torch.float64), newton=(Q, torch.float64), dtheta=(Q * D3, torch.float64),
                  diff=(Q, torch.float64))
    buf = {k: torch.full((shapes[k][0],), 7, dtype=shapes[k][1], device=dev) for k in outs}
    ctx.pair_flip(t(u, np.int32), t(i, np.int32), t(j, np.int32), max_set,
                  None if margin is None else t(margin, np.float64), **buf)
    out = {k: v.cpu().numpy() for k, v in buf.items()}
    for k in ("set_row", "set_val"):
        if k in out:
            out[k] = out[k].reshape(Q, max_set)
    if "dtheta" in out:
        out["dtheta"] = out["dtheta"].reshape(Q, D3)
    return out


@pytest.fixture(scope="module", params=SIZES, ids=lambda v: "%s-k%d" % v)
def case(request, tmp_path_factory):
    model, k = request.param
    c = Case()
    c.model, c.k = model, k
    c.tu, c.ti, c.tr = tu, ti, tr = problem()
    c.p = params_for(model, k)
    c.cases = list(flip_batch(model, k))
    c.cases.append(c.cases[1])                          # the first sized case again, at the end
    c.names = [x["name"] for x in c.cases]
    c.Q = len(c.cases)
    c.u = np.array([x["pair"][0] for x in c.cases], np.int32)
    c.i = np.array([x["pair"][1] for x in c.cases], np.int32)
    c.j = np.array([x["pair"][2] for x in c.cases], np.int32)
    c.margin = np.array([x["margin"] for x in c.cases], np.float64)
    c.refs = [x["ref"] for x in c.cases]
    # test rows 0 .. Q-1 are the cases' (u, i)
    c.m = make_model(model, U, I, k, (tu, ti, tr), (c.u, c.i), c.p, wd=WD, damping=DAMP,
                     tmpdir=tmp_path_factory.mktemp("flip_%s%d" % (model, k)))
    c.fwd = list(range(c.Q))
    c.base = call(c.m.ctx, c.u, c.i, c.j, c.margin, MAX_SET)
    yield c
    c.m.ctx.close()


def same_query(a, qa, b, qb, keys=OUTS):
    """Every output of query qa of result a holds the bits of query qb of result b."""
    for key in keys:
        if key in a and key in b:
            x, y = a[key][qa], b[key][qb]
            same = np.array_equal(x, y) if key in ("set_size", "set_row") else np.array_equal(bits(x), bits(y))
            assert same, (key, qa, qb)


def test_matches_reference(case):
    c = case
    worst = {k: 0.0 for k in ("set_val", "diff", "first_order", "newton", "dtheta")}
    for q, ref in enumerate(c.refs):
        n = ref["set_size"]
        assert n >= 0 and c.base["set_size"][q] == n, (c.names[q], c.base["set_size"][q], n)
        assert np.array_equal(c.base["set_row"][q, :n], ref["set_row"]), c.names[q]
        assert (c.base["set_row"][q, n:] == -1).all() and np.isnan(c.base["set_val"][q, n:]).all()
        one = lambda key: rel_err(c.base[key][q:q + 1], np.array([ref[key]]))
        errs = dict(diff=one("diff"))
        if n == 0:
            # exactly +0.0, without a solve
            assert bits(c.base["first_order"][q:q + 1])[0] == 0 and bits(c.base["newton"][q:q + 1])[0] == 0
            assert (bits(c.base["dtheta"][q]) == 0).all()
        else:
            errs.update(set_val=rel_err(c.base["set_val"][q, :n], ref["set_val"]), first_order=one("first_order"),
                        newton=one("newton"), dtheta=rel_err(c.base["dtheta"][q], ref["dtheta"]))
        print("%s %s margin %.3g size %d rel err %s (cond %.2e)" % (
            c.names[q], c.cases[q]["pair"], c.margin[q], n, {k: "%.1e" % v for k, v in errs.items()}, ref["cond"]))
        for key, err in errs.items():
            worst[key] = max(worst[key], err)
            assert err < RTOL, (c.names[q], key, err)
    print("largest rel err:", {k: "%.2e" % v for k, v in worst.items()})


def test_values_are_the_pair_call_s(case):
    """set_val against get_pair_influence_batch(full=True) at the same positions of the user's list,
    within RTOL of the query's largest pair value (bitwise equality is not claimed)."""
    c = case
    pair = c.m.get_pair_influence_batch(c.fwd, c.j, K=0, full=True, return_x=False)
    worst = 0.0
    for q, ref in enumerate(c.refs):
        n = ref["set_size"]
        if n <= 0:
            continue
        b, e = int(pair["offsets"][q]), int(pair["offsets"][q + 1])
        assert np.array_equal(pair["rel_idx"][b:e][ref["pos"]], c.base["set_row"][q, :n])
        err = np.abs(pair["influence"][b:e][ref["pos"]] - c.base["set_val"][q, :n]).max() / \
            np.abs(pair["influence"][b:e]).max()
        worst = max(worst, err)
        assert err < RTOL, (c.names[q], err)
        assert rel_err(pair["diff"][q:q + 1], c.base["diff"][q:q + 1]) < RTOL
    print("largest |set_val - pair influence| / largest |pair influence|: %.2e" % worst)


def test_first_order_and_newton_disagree_on_the_device(case):
    """Where the reference has first order saying flipped and the re-solved system saying not, the
    device has both verdicts and both signs as the reference has them."""
    c = case
    q = c.names.index("disagree")                       # (flip_batch found one at each of the five sizes)
    ref, mg = c.refs[q], c.margin[q]
    d, fo, nt = c.base["diff"][q], c.base["first_order"][q], c.base["newton"][q]
    print("%s k=%d %s: %d rows, margin %.4g, diff %.4g, first order %.4g (ref %.4g), newton %.4g (ref %.4g)" % (
        c.model, c.k, c.cases[q]["pair"], ref["set_size"], mg, d, fo, ref["first_order"], nt, ref["newton"]))
    assert d + fo < -mg and not d + nt < -mg
    assert ref["diff"] + ref["first_order"] < -mg and not ref["diff"] + ref["newton"] < -mg
    assert np.sign(fo) == np.sign(ref["first_order"]) and np.sign(nt) == np.sign(ref["newton"])


def test_bits(case):
    """Identical bits in every output: a second call; the batch reversed; the first sized case again
    at the end; each output alone through the binding; max_set = 64 against 17 (the same first
    entries; everything, for a set of at most 17 that was not cut); and after prepare_for on exactly
    the batch's (u, i) and (u, j).  Ends with a full prepare."""
    c = case
    ctx = c.m.ctx
    again = call(ctx, c.u, c.i, c.j, c.margin, MAX_SET)
    for q in c.fwd:
        same_query(again, q, c.base, q)
    rev = call(ctx, c.u[::-1], c.i[::-1], c.j[::-1], c.margin[::-1], MAX_SET)
    for q in c.fwd:
        same_query(rev, c.Q - 1 - q, c.base, q)
    assert c.names[1] == c.names[-1] and c.refs[1]["set_size"] > 0
    same_query(c.base, c.Q - 1, c.base, 1)
    for key in OUTS:
        only = call(ctx, c.u, c.i, c.j, c.margin, MAX_SET, outs=(key,))
        for q in c.fwd:
            same_query(only, q, c.base, q, keys=(key,))
    # set_row or set_val without set_size
    two = call(ctx, c.u, c.i, c.j, c.margin, MAX_SET, outs=("set_row", "set_val"))
    for q in c.fwd:
        same_query(two, q, c.base, q)
    small = call(ctx, c.u, c.i, c.j, c.margin, 17)
    whole = 0
    for q, ref in enumerate(c.refs):
        n = min(17, ref["set_size"])
        assert small["set_size"][q] == n
        assert np.array_equal(small["set_row"][q, :n], c.base["set_row"][q, :n])
        assert np.array_equal(bits(small["set_val"][q, :n]), bits(c.base["set_val"][q, :n]))
        assert (small["set_row"][q, n:] == -1).all() and np.isnan(small["set_val"][q, n:]).all()
        if ref["set_size"] <= 17:
            same_query(small, q, c.base, q, keys=("set_size", "first_order", "newton", "dtheta", "diff"))
            whole += 1
    assert whole >= 8
    # the cover of exactly the batch's u, i and j
    c.m.prepare_for(c.fwd, other_items=c.j)
    try:
        sub = call(ctx, c.u, c.i, c.j, c.margin, MAX_SET)
    finally:
        ctx.prepare()
    for q in c.fwd:
        same_query(sub, q, c.base, q)
    # a NULL margin is a margin of 0
    zero = call(ctx, c.u, c.i, c.j, np.zeros(c.Q), MAX_SET)
    none = call(ctx, c.u, c.i, c.j, None, MAX_SET)
    for q in c.fwd:
        same_query(none, q, zero, q)


def test_bad_queries_through_the_binding(case):
    """Ids out of range (-1, U, I, 2^31 - 1), i == j and n == 0 given to the binding directly (the
    facade refuses them): never an index, set_size -1 and NaN in every double output but diff (NaN for
    a bad id, +0.0 for i == j, the gap for n == 0), empty slots -- and the neighbours keep their bits.
    Then the checks of the call."""
    import torch
    c = case
    ctx, dev = c.m.ctx, c.m.ctx.torch_device
    big = 2 ** 31 - 1
    a, b = 1, c.names.index("exhausted")
    (u0, i0, j0), (u1, i1, j1) = c.cases[a]["pair"], c.cases[b]["pair"]
    us = [u0, -1, U, u0, u1, u0, big, u0, 19, u0]
    iis = [i0, i0, i0, I, i1, i0, i0, big, 318, i0]
    js = [j0, j0, j0, j0, j1, i0, j0, j0, 319, -1]
    mg = [c.margin[a]] * 4 + [c.margin[b]] + [c.margin[a]] * 5
    live = {0: a, 4: b}
    got = call(ctx, us, iis, js, mg, MAX_SET)
    for row in range(len(us)):
        if row in live:
            same_query(got, row, c.base, live[row])
            continue
        assert got["set_size"][row] == -1
        assert (got["set_row"][row] == -1).all() and np.isnan(got["set_val"][row]).all()
        assert np.isnan(got["first_order"][row]) and np.isnan(got["newton"][row]) and np.isnan(got["dtheta"][row]).all()
        if row == 5:                                    # i == j
            assert bits(got["diff"][row:row + 1])[0] == 0
        elif row == 8:                                  # n == 0
            assert np.isfinite(got["diff"][row])
        else:
            assert np.isnan(got["diff"][row])
    # the argument checks
    for max_set in (0, FIA_FLIP_MAX_SET + 1):
        with pytest.raises(FIAError, match="invalid argument.*max_set"):
            call(ctx, c.u, c.i, c.j, c.margin, max_set, outs=("set_size",))
    with pytest.raises(FIAError, match="invalid argument.*no output"):
        call(ctx, c.u, c.i, c.j, c.margin, MAX_SET, outs=())
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v, np.int32)).to(dev)
    qu, qi, qj = t(c.u), t(c.i), t(c.j)
    size = torch.zeros(c.Q, dtype=torch.int32, device=dev)
    ptr = lambda x: None if x is None else x.data_ptr()
    for ids in ((None, qi, qj), (qu, None, qj), (qu, qi, None)):
        rc = ctx.lib.fia_pair_flip(ctx.h, c.Q, ptr(ids[0]), ptr(ids[1]), ptr(ids[2]), None, 16, size.data_ptr(), None,
                                   None, None, None, None, None, None)
        assert rc == 1                                  # FIA_ERR_INVALID
    assert ctx.lib.fia_pair_flip(ctx.h, 0, None, None, None, None, 16, size.data_ptr(), None, None, None, None, None,
                                 None, None) == 0      # an empty batch launches nothing
    # a cover without the j's: the facade's count refuses the batch (FIA_ERR_STATE)
    c.m.prepare_for(c.fwd)
    try:
        with pytest.raises(FIAError, match="bad call order"):
            c.m.get_flip_sets(c.fwd, c.j, margin=c.margin, max_set=MAX_SET)
    finally:
        ctx.prepare()
    same_query(call(ctx, c.u[:3], c.i[:3], c.j[:3], c.margin[:3], MAX_SET), 1, c.base, 1)


def test_facade(case):
    """get_flip_sets equals the binding; get_counterfactual_explanation on user 0's test rating with
    three alternatives returns the smallest flipping set under both settings of `verified`, compared
    with the same loop run on flip_reference."""
    c = case
    res = c.m.get_flip_sets(c.fwd, c.j, margin=c.margin, max_set=MAX_SET, return_dtheta=True)
    for key in ("diff", "first_order", "newton", "dtheta"):
        assert np.array_equal(bits(res[key]), bits(c.base[key])), key
    assert np.array_equal(res["set_size"], c.base["set_size"]) and res["set_size"].dtype == np.int64
    for q in c.fwd:
        n = c.base["set_size"][q]
        assert res["sets"][q].shape == (n,) and np.array_equal(res["sets"][q], c.base["set_row"][q, :n])
        assert np.array_equal(bits(res["set_vals"][q]), bits(c.base["set_val"][q, :n]))
    assert np.array_equal(res["flipped_first_order"], c.base["diff"] + c.base["first_order"] < -c.margin)
    assert np.array_equal(res["flipped_newton"], c.base["diff"] + c.base["newton"] < -c.margin)
    assert "dtheta" not in c.m.get_flip_sets(c.fwd[:2], c.j[:2])
    # ACCENT's outer loop
    cf = [c.names.index(nm) for nm in ("cf_8", "cf_318", "cf_40")]
    assert all(c.cases[q]["pair"][:2] == (0, 7) for q in cf)
    alts = [c.cases[q]["pair"][2] for q in cf]
    for verified in (True, False):
        want = -1
        for a, q in enumerate(cf):
            r = c.refs[q]
            flips = r["diff"] + (r["newton"] if verified else r["first_order"]) < -CF_MARGIN
            if flips and (want < 0 or r["set_size"] < c.refs[cf[want]]["set_size"]):
                want = a
        got = c.m.get_counterfactual_explanation(cf[0], alts, margin=CF_MARGIN, max_set=MAX_SET, verified=verified)
        print("%s k=%d verified=%s: alternative %s, rows %s" % (c.model, c.k, verified, got["item"], got["rows"]))
        assert got["index"] == want and len(got["table"]["sets"]) == 3
        if want < 0:
            assert got["item"] is None and got["rows"] is None
        else:
            assert got["item"] == alts[want] and np.array_equal(got["rows"], c.refs[cf[want]]["set_row"])
    if not verified:
        assert want >= 0                                # to first order every closed set flips


@pytest.mark.parametrize("model,k", [("MF", 64), ("NCF", 32)])
def test_other_sizes_are_unsupported(model, k, tmp_path):
    """MF k=64 and NCF k=32: FIA_ERR_UNSUPPORTED through the facade, naming the built sizes."""
    tu, ti, tr = problem()
    qs = pair_list(tu, ti)[:2]
    qu = np.array([q[0] for q in qs], np.int32)
    qi = np.array([q[1] for q in qs], np.int32)
    m = make_model(model, U, I, k, (tu, ti, tr), (qu, qi), params_for(model, k), wd=WD, damping=DAMP, tmpdir=tmp_path)
    try:
        with pytest.raises(FIAError, match="unsupported.*MF k in \\{8, 16, 32\\} and NCF k in \\{8, 16\\}"):
            m.get_flip_sets([0, 1], [q[2] for q in qs])
    finally:
        m.ctx.close()
