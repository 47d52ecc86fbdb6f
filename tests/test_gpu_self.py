"""GPU tests of fia_self_influence / get_self_influence: every train row's effect on its own
prediction.  For train row j = (a, b, y), with v, H, theta_t and n of the query (a, b),

    b_j = (2/n) (2 e v + wd M theta_t),   H_j = (2/n) (2 v v^T + 2 e C + wd M)
    first_order = (H^-1 v) . b_j,   newton = v . (H - H_j)^-1 b_j,   error = e = r-hat(a, b) - y

against group_reference (tests/test_group_cpu.py) of the query (a, b) with the single group {j},
against fia_group_influence on the GPU (the merged kernel checks the fused one), and for the
properties of the call: position independence, determinism, bad rows, top-K, state.

Tolerance: the project's RTOL = 1e-5 relative to the largest |want| (rel_err) over the batch.
Both sides solve in fp64, so the error is about eps * cond(H - H_j); every compared row is
asserted (on the CPU) to leave cond(H - H_j) < COND_MAX = 1e8, which keeps that under 1e-7.

The problem is test_gpu_group's: 12 users, 128 items, 418 ratings; user 0 rates items 0 .. 125,
of which 40 .. 125 have no other rating (item 41 has user 10's too) -- an item side of one
rating; the pair (3, 5) is present twice with different ratings; user 10 has three ratings."""
import numpy as np
import pytest

from influence import _lib, synth
from test_group_cpu import group_reference, w3g_of
from test_gpu_group import COND_MAX, DAMP, I, SIZES, U, WD, problem
from test_gpu_parity import RTOL, make_model, rel_err

pytestmark = pytest.mark.gpu

DUP = (3, 5)
KEYS = ("first_order", "newton", "error")


def compared_rows(tu, ti, k):
    """All rows at k = 8; else a fixed subset: both rows of the duplicated pair, user 10's three,
    22 rows of the heavy user on items nobody else rated, 22 rows with at least 4 ratings on each
    side, and every 31st row."""
    n = len(tu)
    if k == 8:
        return np.arange(n)
    du, di = np.bincount(tu, minlength=U), np.bincount(ti, minlength=I)
    dup = np.nonzero((tu == DUP[0]) & (ti == DUP[1]))[0]
    u10 = np.nonzero(tu == 10)[0]
    single = np.nonzero((tu == 0) & (di[ti] == 1))[0][:22]
    both4 = np.nonzero((du[tu] >= 4) & (di[ti] >= 4))[0][:22]
    assert dup.size == 2 and u10.size == 3 and single.size == 22 and both4.size == 22
    return np.unique(np.concatenate([dup, u10, single, both4, np.arange(0, n, 31)]))


def reference(model, p, k, tu, ti, tr, rows):
    """Per compared row: first_order, newton (the reference's `group`), error, cond(H - H_j)."""
    from oracle import fia_oracle as fo
    W3g = w3g_of(model, p, k)
    out = {key: np.empty(len(rows)) for key in KEYS + ("cond",)}
    cores = {}
    for t, j in enumerate(rows):
        pair = (int(tu[j]), int(ti[j]))
        if pair not in cores:                            # (the duplicated pair's rows share a query)
            cores[pair] = fo.query(model, p, k, tu, ti, tr, pair[0], pair[1], WD, DAMP)
        core = cores[pair]
        ref = group_reference(core, [int(j)], WD, DAMP, W3g)
        occ = np.nonzero(core["rel"] == j)[0]
        assert occ.size == 2
        out["first_order"][t], out["newton"][t] = ref["first_order"], ref["group"]
        out["error"][t], out["cond"][t] = core["e"][occ[0]], ref["cond"]
    return out


def np_topk(vals, K):
    """(pos, val) of the K entries of largest |v|: ties to the lower position, NaN last, -1 / NaN
    in unused slots."""
    vals = np.asarray(vals, np.float64)
    key = np.where(np.isnan(vals), -1.0, np.abs(vals))
    order = np.lexsort((np.arange(vals.size), -key))[:K]
    pos = np.full(K, -1, np.int64)
    val = np.full(K, np.nan)
    pos[:order.size], val[:order.size] = order, vals[order]
    return pos, val


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


class Case(object):
    pass


@pytest.fixture(scope="module", params=SIZES, ids=lambda v: "%s-k%d" % v)
def case(request, tmp_path_factory):
    model, k = request.param
    c = Case()
    c.model, c.k = model, k
    c.tu, c.ti, c.tr = tu, ti, tr = problem()
    c.n = len(tr)
    c.p = synth.mf_params(U, I, k, 3) if model == "MF" else synth.ncf_params(U, I, k, 3)
    # the test pairs are the train pairs: test index j is the query of train row j (the group call)
    c.m = make_model(model, U, I, k, (tu, ti, tr), (tu, ti), c.p, wd=WD, damping=DAMP,
                     tmpdir=tmp_path_factory.mktemp("self_%s%d" % (model, k)))
    c.rows = compared_rows(tu, ti, k)
    c.ref = reference(model, c.p, k, tu, ti, tr, c.rows)
    c.base = c.m.get_self_influence(K=4)
    yield c
    c.m.ctx.close()


def test_compared_rows_are_well_conditioned(case):
    """Every compared row leaves cond(H - H_j) < 1e8 (all 418 rows at k = 8), so RTOL is a
    meaningful bound (eps * cond < 1e-7).  No row is left out for its conditioning."""
    c = case
    if c.k == 8:
        assert c.rows.size == c.n == 418
    else:
        du, di = np.bincount(c.tu, minlength=U), np.bincount(c.ti, minlength=I)
        r = c.rows
        assert 55 <= r.size <= 75
        assert ((c.tu[r] == DUP[0]) & (c.ti[r] == DUP[1])).sum() == 2 and (c.tu[r] == 10).sum() == 3
        assert ((c.tu[r] == 0) & (di[c.ti[r]] == 1)).sum() >= 20
        assert ((du[c.tu[r]] >= 4) & (di[c.ti[r]] >= 4)).sum() >= 20
    worst = int(np.argmax(c.ref["cond"]))
    print("largest cond(H - H_j) %.3e at row %d" % (c.ref["cond"][worst], c.rows[worst]))
    assert (c.ref["cond"] < COND_MAX).all(), (c.rows[worst], c.ref["cond"][worst])


def test_matches_reference(case):
    c = case
    res = c.base
    assert res["rows"].dtype == np.int64 and np.array_equal(res["rows"], np.arange(c.n))
    for key in KEYS:
        assert res[key].shape == (c.n,) and res[key].dtype == np.float64 and np.isfinite(res[key]).all(), key
        err = rel_err(res[key][c.rows], c.ref[key])
        print("rel err %s %.2e (largest |want| %.3e)" % (key, err, np.abs(c.ref[key]).max()))
        assert err < RTOL, key
    # the row's own curvature is not negligible: newton is not first_order
    gap = np.abs(c.ref["newton"] - c.ref["first_order"]) / np.abs(c.ref["first_order"])
    print("largest |newton - first_order| / |first_order| %.3e" % gap.max())
    assert (gap > 100 * RTOL).any()
    # the two rows of the duplicated pair: m = 2 each, their own y
    d = np.nonzero((c.tu == DUP[0]) & (c.ti == DUP[1]))[0]
    assert res["error"][d[0]] != res["error"][d[1]] and res["newton"][d[0]] != res["newton"][d[1]]


def test_matches_group_call_on_the_gpu(case):
    """fia_group_influence with every train pair as a query and the singleton group {j}: the
    merged kernel against the fused one, all 418 rows."""
    c = case
    grp = c.m.get_group_influence(list(range(c.n)), [[np.array([j])] for j in range(c.n)])
    ef = rel_err(c.base["first_order"], grp["first_order"])
    en = rel_err(c.base["newton"], grp["group"])
    print("rel err against the group call: first_order %.2e newton %.2e" % (ef, en))
    assert np.isfinite(grp["group"]).all() and np.isfinite(grp["first_order"]).all()
    assert ef < RTOL and en < RTOL


def test_position_independent_and_deterministic(case):
    """Bitwise: a second call; None against arange; reversed; a subset with a row twice; 12
    repetitions of all rows (5016 positions: more than the 256 x 16 workgroups a launch can
    have, so the grid-stride loop runs)."""
    c = case
    base = c.base
    again = c.m.get_self_influence(K=4)
    listed = c.m.get_self_influence(np.arange(c.n))
    rev = c.m.get_self_influence(np.arange(c.n)[::-1].copy())
    sub_rows = np.array([7, 300, 7, 0, c.n - 1, 150, 300])
    sub = c.m.get_self_influence(sub_rows)
    many = c.m.get_self_influence(np.tile(np.arange(c.n), 12))
    assert many["newton"].shape == (12 * c.n,) and 12 * c.n > 256 * 16
    assert np.array_equal(sub["rows"], sub_rows)
    for key in KEYS:
        assert same_bits(again[key], base[key]), key
        assert same_bits(listed[key], base[key]), key
        assert same_bits(rev[key][::-1], base[key]), key
        assert same_bits(sub[key], base[key][sub_rows]), key
        assert same_bits(many[key], np.tile(base[key], 12)), key
    for key in ("topk_pos", "topk_idx"):
        assert np.array_equal(again[key], base[key]), key
    assert same_bits(again["topk_val"], base["topk_val"])


def test_bad_rows_through_the_binding(case):
    """Rows outside [0, n_train), given to Context.self_influence directly (the facade would
    refuse them): NaN in all three outputs at those slots, the neighbours keep their bits, and
    in the top-K the NaN positions rank last."""
    import torch
    c = case
    ctx = c.m.ctx
    dev = ctx.torch_device
    rows = np.array([5, 17, c.n, 200, -1, 33, 2 ** 31 - 1, c.n - 1, 5], np.int64)
    bad = np.array([2, 4, 6])
    good = np.setdiff1d(np.arange(rows.size), bad)
    d_rows = torch.from_numpy(rows.astype(np.int32)).to(dev)
    out = [torch.full((rows.size,), 7.0, dtype=torch.float64, device=dev) for _ in range(3)]
    ctx.self_influence(d_rows, out[0], out[1], out[2])
    for key, t in zip(KEYS, out):
        got = t.cpu().numpy()
        assert np.isnan(got[bad]).all(), key
        assert same_bits(got[good], c.base[key][rows[good]]), key
    # two good rows and three bad ones, K = 4: the good ones by |newton|, then NaN by position
    short = np.array([5, c.n, 200, -1, 2 ** 31 - 1], np.int64)
    d_short = torch.from_numpy(short.astype(np.int32)).to(dev)
    newton = torch.empty(short.size, dtype=torch.float64, device=dev)
    tp = torch.empty(4, dtype=torch.int64, device=dev)
    ti = torch.empty(4, dtype=torch.int64, device=dev)
    tv = torch.empty(4, dtype=torch.float64, device=dev)
    ctx.self_influence(d_short, None, newton, None, 4, tp, ti, tv)
    want_pos, want_val = np_topk(newton.cpu().numpy(), 4)
    assert sorted(want_pos[:2].tolist()) == [0, 2] and want_pos[2:].tolist() == [1, 3]
    assert np.array_equal(tp.cpu().numpy(), want_pos)
    assert np.array_equal(ti.cpu().numpy(), short[want_pos])
    assert same_bits(tv.cpu().numpy(), want_val) and np.isnan(want_val[2:]).all()


def test_topk(case):
    """Exact against numpy on the call's own newton values, under the tie rule."""
    c = case
    for K in (1, 4, 64):
        res = c.base if K == 4 else c.m.get_self_influence(K=K)
        pos, val = np_topk(res["newton"], K)
        assert res["topk_pos"].dtype == np.int64 and res["topk_idx"].dtype == np.int64
        assert np.array_equal(res["topk_pos"], pos), K
        assert np.array_equal(res["topk_idx"], pos), K               # every row in order: row = position
        assert same_bits(res["topk_val"], val), K
        assert same_bits(res["newton"], c.base["newton"])
        # a NULL newton: the values go to scratch, the same top-K comes back
        lean = c.m.get_self_influence(K=K, full=False)
        assert sorted(lean) == ["topk_idx", "topk_pos", "topk_val"]
        assert np.array_equal(lean["topk_pos"], pos) and np.array_equal(lean["topk_idx"], pos)
        assert same_bits(lean["topk_val"], val)
    # a permuted list: topk_idx is the train row, topk_pos the position in the list
    perm = np.random.default_rng(5).permutation(c.n)
    res = c.m.get_self_influence(perm, K=4)
    pos, val = np_topk(res["newton"], 4)
    assert np.array_equal(res["topk_pos"], pos) and np.array_equal(res["topk_idx"], perm[pos])
    assert same_bits(res["topk_val"], val)
    # fewer rows than K: the last slot is empty
    three = c.m.get_self_influence(np.array([9, 2, 250]), K=4)
    pos, val = np_topk(three["newton"], 4)
    assert pos[3] == -1 and np.isnan(val[3])
    assert np.array_equal(three["topk_pos"], pos) and same_bits(three["topk_val"], val)
    assert three["topk_idx"].tolist() == [[9, 2, 250][t] for t in pos[:3]] + [-1]
    # one row twice: equal values, the lower position first
    top = int(c.base["topk_idx"][0])
    r0, r1 = [r for r in (3, 8, 11) if r != top][:2]
    twice = c.m.get_self_influence(np.array([r0, top, r1, top]), K=4)
    assert twice["topk_pos"][:2].tolist() == [1, 3] and twice["topk_idx"][:2].tolist() == [top, top]
    assert np.array_equal(twice["topk_pos"], np_topk(twice["newton"], 4)[0])


def test_empty_batch_and_state(case):
    """num_rows == 0: empty arrays, the top-K slots filled.  After prepare_for the call refuses
    (a partial cover); after a full prepare it answers with the same bits.  Runs last on the
    model."""
    c = case
    none = c.m.get_self_influence(np.zeros(0, np.int64), K=4)
    for key in KEYS:
        assert none[key].shape == (0,)
    assert none["rows"].shape == (0,)
    assert none["topk_pos"].tolist() == [-1] * 4 and none["topk_idx"].tolist() == [-1] * 4
    assert np.isnan(none["topk_val"]).all()
    c.m.prepare_for([0, 1, 2])
    try:
        with pytest.raises(_lib.FIAError, match="prepare"):
            c.m.get_self_influence(K=4)
    finally:
        c.m.ctx.prepare()
    back = c.m.get_self_influence(K=4)
    for key in KEYS + ("topk_val",):
        assert same_bits(back[key], c.base[key]), key
    assert np.array_equal(back["topk_pos"], c.base["topk_pos"])
