"""GPU tests of fia_self_influence / get_self_influence at the large-k sizes: every listed train
row's effect on its own prediction, the systems in device memory.  A row's own downdate needs no
slab (dA_u = v_u v_u^T, dB_i = v_i v_i^T, c_S = 1, e_S = e, m_S = 2); the rows run in chunks whose
per-row work words bound the scratch.

The problem is that of tests/test_gpu_group.py (12 users, 128 items, 418 ratings, the pair (3, 5)
twice).  MF 128 and NCF 64 compare all 418 rows; MF 256 and NCF 128 compare 32 rows that include
both rows of the duplicated pair and rows of the heavy user.

Tolerance: the project's RTOL = 1e-5 relative to the largest |want| (rel_err) over the batch, as in
tests/test_gpu_self.py: both sides solve in fp64 and every compared row is asserted (on the CPU) to
leave cond(H - H_j) < COND_MAX = 1e8, so eps * cond stays under 1e-7."""
import os

import numpy as np
import pytest

from influence import _lib, synth
from test_group_cpu import w3g_of
from test_self_cpu import self_reference
from test_gpu_group import COND_MAX, DAMP, I, U, WD, problem
from test_gpu_self import DUP, KEYS, np_topk, same_bits
from test_gpu_parity import RTOL, make_model, rel_err

pytestmark = pytest.mark.gpu

SIZES = [("MF", 128, True), ("NCF", 64, True), ("MF", 256, False), ("NCF", 128, False)]


class Case(object):
    pass


def compared_rows(tu, ti, every):
    n = len(tu)
    if every:
        return np.arange(n)
    dup = np.nonzero((tu == DUP[0]) & (ti == DUP[1]))[0]
    heavy = np.nonzero(tu == 0)[0][:6]
    u10 = np.nonzero(tu == 10)[0]
    must = np.unique(np.concatenate([dup, heavy, u10]))
    fill = np.setdiff1d(np.arange(3, n, 13), must)[:32 - must.size]
    rows = np.sort(np.concatenate([must, fill]))
    assert rows.size == 32 and np.unique(rows).size == 32 and np.isin(dup, rows).all() and (tu[rows] == 0).any()
    return rows


@pytest.fixture(scope="module", params=SIZES, ids=lambda v: "%s-k%d" % v[:2])
def case(request, tmp_path_factory):
    model, k, every = request.param
    c = Case()
    c.model, c.k, c.every = model, k, every
    c.tu, c.ti, c.tr = tu, ti, tr = problem()
    c.n = len(tr)
    c.p = synth.mf_params(U, I, k, 3) if model == "MF" else synth.ncf_params(U, I, k, 3)
    c.m = make_model(model, U, I, k, (tu, ti, tr), (tu, ti), c.p, wd=WD, damping=DAMP,
                     tmpdir=tmp_path_factory.mktemp("self_big_%s%d" % (model, k)))
    c.rows = compared_rows(tu, ti, every)
    W3g = w3g_of(model, c.p, k)
    c.ref = {key: np.empty(c.rows.size) for key in KEYS + ("cond",)}
    for t, j in enumerate(c.rows):
        first, newton, e, cond, _, _ = self_reference(model, c.p, k, tu, ti, tr, int(j), WD, DAMP, W3g)
        c.ref["first_order"][t], c.ref["newton"][t], c.ref["error"][t], c.ref["cond"][t] = first, newton, e, cond
    c.base = c.m.get_self_influence(c.rows, K=4)
    yield c
    c.m.ctx.close()


def test_compared_rows_are_well_conditioned(case):
    c = case
    worst = int(np.argmax(c.ref["cond"]))
    print("largest cond(H - H_j) %.3e at row %d" % (c.ref["cond"][worst], c.rows[worst]))
    assert (c.ref["cond"] < COND_MAX).all(), (c.rows[worst], c.ref["cond"][worst])
    assert c.rows.size == (c.n if c.every else 32)


def test_matches_reference(case):
    c = case
    res = c.base
    assert np.array_equal(res["rows"], c.rows)
    for key in KEYS:
        assert res[key].shape == (c.rows.size,) and np.isfinite(res[key]).all(), key
        err = rel_err(res[key], c.ref[key])
        print("rel err %s %.2e (largest |want| %.3e)" % (key, err, np.abs(c.ref[key]).max()))
        assert err < RTOL, key
    gap = np.abs(c.ref["newton"] - c.ref["first_order"]) / np.abs(c.ref["first_order"])
    assert (gap > 100 * RTOL).any()
    d = np.nonzero((c.tu[c.rows] == DUP[0]) & (c.ti[c.rows] == DUP[1]))[0]
    assert d.size == 2
    assert res["error"][d[0]] != res["error"][d[1]] and res["newton"][d[0]] != res["newton"][d[1]]


def test_matches_group_call_on_the_gpu(case):
    """fia_group_influence with the row's pair as the query and the singleton group {j}."""
    c = case
    grp = c.m.get_group_influence([int(j) for j in c.rows], [[np.array([j])] for j in c.rows])
    ef = rel_err(c.base["first_order"], grp["first_order"])
    en = rel_err(c.base["newton"], grp["group"])
    print("rel err against the group call: first_order %.2e newton %.2e" % (ef, en))
    assert np.isfinite(grp["group"]).all() and np.isfinite(grp["first_order"]).all()
    assert ef < RTOL and en < RTOL


def test_topk_none_and_positions(case):
    """K = 4 under the tie rule, exact against numpy on the call's own newton values; rows=None is
    every row in order; a row's values do not depend on where it sits or on the batch."""
    c = case
    pos, val = np_topk(c.base["newton"], 4)
    assert np.array_equal(c.base["topk_pos"], pos) and np.array_equal(c.base["topk_idx"], c.rows[pos])
    assert same_bits(c.base["topk_val"], val)
    lean = c.m.get_self_influence(c.rows, K=4, full=False)
    assert np.array_equal(lean["topk_pos"], pos) and same_bits(lean["topk_val"], val)
    every = c.m.get_self_influence(K=4)
    assert np.array_equal(every["rows"], np.arange(c.n))
    for key in KEYS:
        assert every[key].shape == (c.n,) and np.isfinite(every[key]).all(), key
        assert same_bits(every[key][c.rows], c.base[key]), key
    p2, v2 = np_topk(every["newton"], 4)
    assert np.array_equal(every["topk_pos"], p2) and np.array_equal(every["topk_idx"], p2)
    assert same_bits(every["topk_val"], v2)
    rev = c.m.get_self_influence(c.rows[::-1].copy())
    again = c.m.get_self_influence(c.rows, K=4)
    for key in KEYS:
        assert same_bits(rev[key][::-1], c.base[key]), key
        assert same_bits(again[key], c.base[key]), key


def test_two_chunks_give_the_bits_of_one(case):
    """The chunk limit lowered through the implementation's testing knob (FIA_BIGK_CHUNK), so the
    batch needs two chunks (32 rows) or more."""
    c = case
    os.environ["FIA_BIGK_CHUNK"] = "20"
    try:
        chunked = c.m.get_self_influence(c.rows, K=4)
    finally:
        del os.environ["FIA_BIGK_CHUNK"]
    assert c.rows.size > 20
    for key in KEYS + ("topk_val",):
        assert same_bits(chunked[key], c.base[key]), key
    assert np.array_equal(chunked["topk_pos"], c.base["topk_pos"])


def test_bad_rows_through_the_binding(case):
    """Rows outside [0, n_train): NaN in all three outputs at those slots, the neighbours keep
    their bits."""
    import torch
    c = case
    ctx = c.m.ctx
    dev = ctx.torch_device
    r = c.rows
    rows = np.array([r[0], r[5], c.n, r[9], -1, r[1], 2 ** 31 - 1, r[-1], r[0]], np.int64)
    where = {int(j): t for t, j in enumerate(r)}
    bad = np.array([2, 4, 6])
    good = np.setdiff1d(np.arange(rows.size), bad)
    d_rows = torch.from_numpy(rows.astype(np.int32)).to(dev)
    out = [torch.full((rows.size,), 7.0, dtype=torch.float64, device=dev) for _ in range(3)]
    ctx.self_influence(d_rows, out[0], out[1], out[2])
    for key, t in zip(KEYS, out):
        got = t.cpu().numpy()
        assert np.isnan(got[bad]).all(), key
        assert same_bits(got[good], c.base[key][[where[int(j)] for j in rows[good]]]), key


def test_state_after_prepare_for(case):
    """After prepare_for the call refuses (a partial cover); after a full prepare it answers with
    the same bits.  Runs last on the model."""
    c = case
    c.m.prepare_for([0, 1, 2])
    try:
        with pytest.raises(_lib.FIAError, match="prepare"):
            c.m.get_self_influence(c.rows, K=4)
    finally:
        c.m.ctx.prepare()
    back = c.m.get_self_influence(c.rows, K=4)
    for key in KEYS + ("topk_val",):
        assert same_bits(back[key], c.base[key]), key
