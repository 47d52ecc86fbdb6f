"""GPU tests of fia_group_influence / get_group_influence at the large-k sizes (MF k in {128,
256}, NCF k in {64, 128, 256}), where the systems live in device memory: the downdated coupled
system H - H_S is the base system of the per-query solver with two Gram-shaped downdates and four
scalars changed (tests/test_group_bigk_cpu.py), solved by the same blocked LDL^T.

The problem, queries and groups are those of tests/test_gpu_group.py (12 users, 128 items, 418
ratings).  MF 128 (side blocks of 129 coordinates padded to 144) and NCF 64 (128, no padding) run
every query and group, plus user-side groups of exactly 16 and 17 members (one full slab of the
MFMA staging; a full slab and a tail of one).  MF 256, NCF 128 and NCF 256 run query 0 with the
groups "one", "mixed", "own", "wide", "empty" against the reference (and "user" with and without
unrelated rows for the bitwise properties), which keeps the oracle's 1024 x 1024 solves to a few.

Tolerance: the project's RTOL = 1e-5 relative to the largest |want| (rel_err), for group and
first_order over the batch and for dtheta per group.  Both sides solve in fp64, so the error is
about eps * cond(H - H_S); every compared group is asserted (on the CPU) to leave a condition
number below COND_MAX = 1e8, which keeps that under 1e-7."""
import os

import numpy as np
import pytest

from influence import synth
from test_group_cpu import group_reference, w3g_of
from test_gpu_group import COND_MAX, DAMP, I, U, WD, build_groups, problem, queries
from test_gpu_parity import RTOL, make_model, rel_err

pytestmark = pytest.mark.gpu

FULL = [("MF", 128), ("NCF", 64)]
REDUCED = [("MF", 256), ("NCF", 128), ("NCF", 256)]
REDUCED_REF = ("one", "mixed", "own", "wide", "empty")
REDUCED_RUN = REDUCED_REF + ("user", "user+unrelated")
KEYS = ("group", "first_order", "dtheta")


class Case(object):
    pass


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


@pytest.fixture(scope="module", params=FULL + REDUCED, ids=lambda v: "%s-k%d" % v)
def case(request, tmp_path_factory):
    from oracle import fia_oracle as fo
    model, k = request.param
    c = Case()
    c.model, c.k = model, k
    c.full = (model, k) in FULL
    c.tu, c.ti, c.tr = tu, ti, tr = problem()
    c.p = synth.mf_params(U, I, k, 3) if model == "MF" else synth.ncf_params(U, I, k, 3)
    qs = queries(tu, ti)
    named = build_groups(tu, ti, qs)
    if c.full:
        (u0, i0) = qs[0]
        user_side = np.nonzero((tu == u0) & (ti != i0))[0]
        named[0] = named[0] + [("u16", user_side[:16]), ("u17", user_side[20:37])]
        want_ref = lambda q, name: True
    else:
        qs = qs[:1]
        named = [[(n, r) for n, r in named[0] if n in REDUCED_RUN]]
        want_ref = lambda q, name: name in REDUCED_REF
    c.qs, c.named = qs, named
    c.groups = [[np.asarray(r, np.int64) for _, r in per] for per in named]
    c.flat = [r for per in c.groups for r in per]
    qu = np.array([q[0] for q in qs], np.int32)
    qi = np.array([q[1] for q in qs], np.int32)
    c.m = make_model(model, U, I, k, (tu, ti, tr), (qu, qi), c.p, wd=WD, damping=DAMP,
                     tmpdir=tmp_path_factory.mktemp("group_big_%s%d" % (model, k)))
    c.D = fo.num_params(model, k)
    W3g = w3g_of(model, c.p, k)
    c.cores = [fo.query(model, c.p, k, tu, ti, tr, u, i, WD, DAMP) for (u, i) in qs]
    # the reference, once: per group (query, name, reference or None where n_q = 0 / not compared)
    c.refs = []
    for q, per in enumerate(named):
        for name, rows in per:
            ref = group_reference(c.cores[q], rows, WD, DAMP, W3g) if c.cores[q]["n"] and want_ref(q, name) else None
            c.refs.append((q, name, ref))
    c.res = c.m.get_group_influence(list(range(len(qs))), c.groups, return_dtheta=True)
    yield c
    c.m.ctx.close()


def gid(c, q, name):
    return next(g for g, (qq, nn, _) in enumerate(c.refs) if qq == q and nn == name)


def test_groups_are_well_conditioned(case):
    c = case
    worst = 0.0
    for (q, name, ref), rows in zip(c.refs, c.flat):
        if ref is None or rows.size == 0:
            continue
        worst = max(worst, ref["cond"])
        assert ref["cond"] < COND_MAX, (q, name, ref["cond"])
    print("largest cond(H - H_S) %.3e" % worst)
    if c.full:
        assert {len(c.flat[gid(c, 0, n)]) for n in ("u16", "u17")} == {16, 17}


def test_matches_reference(case):
    c = case
    res = c.res
    G = len(c.refs)
    assert res["group"].shape == (G,) and res["first_order"].shape == (G,) and res["dtheta"].shape == (G, c.D)
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
    if c.full:
        # the group of 20: the corrected value is the reference's and not the first-order sum
        ref = c.refs[gid(c, 0, "twenty")][2]
        g20 = gid(c, 0, "twenty")
        assert abs(res["group"][g20] - ref["group"]) < RTOL * abs(ref["group"])
        assert abs(res["first_order"][g20] - ref["first_order"]) < RTOL * abs(ref["first_order"])
        assert abs(ref["group"] - ref["first_order"]) > 0.035 * abs(ref["first_order"])


def test_empty_group_unrelated_rows_and_no_related_ratings(case):
    """+0.0 for an empty group; a group with unrelated rows mixed in (more than 64 listed members)
    is bitwise the group alone; n_q = 0 gives NaN, the empty group of that query included."""
    c = case
    res = c.res
    ge = gid(c, 0, "empty")
    assert bits(res["group"][ge:ge + 1])[0] == 0 and bits(res["first_order"][ge:ge + 1])[0] == 0
    assert (bits(res["dtheta"][ge]) == 0).all()
    a, b = gid(c, 0, "user"), gid(c, 0, "user+unrelated")
    for key in KEYS:
        assert np.array_equal(bits(res[key][a]), bits(res[key][b])), key
    assert res["group"][a] != 0.0 and np.isfinite(res["dtheta"][a]).all()
    if c.full:
        for name in ("nq0", "nq0-empty"):
            g = gid(c, 5, name)
            assert np.isnan(res["group"][g]) and np.isnan(res["first_order"][g]) and np.isnan(res["dtheta"][g]).all()


def test_position_independent_and_deterministic(case):
    """A second identical call, the batch reversed, the batch in chunks of three groups, and (all
    queries) the same group of the same pair later in the batch: the same bits."""
    c = case
    res = c.res
    Q = len(c.qs)
    again = c.m.get_group_influence(list(range(Q)), c.groups, return_dtheta=True)
    for key in KEYS:
        assert np.array_equal(bits(res[key]), bits(again[key])), key
    order = list(range(Q))[::-1]
    rev = c.m.get_group_influence(order, [c.groups[q][::-1] for q in order], return_dtheta=True)
    for key in KEYS:
        assert np.array_equal(bits(rev[key][::-1]), bits(res[key])), key
    os.environ["FIA_BIGK_CHUNK"] = "3"
    try:
        chunked = c.m.get_group_influence(list(range(Q)), c.groups, return_dtheta=True)
    finally:
        del os.environ["FIA_BIGK_CHUNK"]
    assert len(c.refs) > 3
    for key in KEYS:
        assert np.array_equal(bits(chunked[key]), bits(res[key])), key
    if c.full:
        a, b = gid(c, 0, "user"), gid(c, 6, "user")
        for key in KEYS:
            assert np.array_equal(bits(res[key][a]), bits(res[key][b])), key


def test_bad_row_and_null_outputs_through_the_binding(case):
    """A member row outside [0, n_train): NaN for that group only, its neighbours keep their bits.
    Each output may be NULL: the others keep their bits."""
    import torch
    c = case
    ctx = c.m.ctx
    dev = ctx.torch_device
    n_train = len(c.tr)
    a = gid(c, 0, "user")
    user = c.flat[a]
    t = lambda arr, dt: torch.from_numpy(np.ascontiguousarray(arr, dt)).to(dev)
    qu, qi = t([c.qs[0][0]], np.int32), t([c.qs[0][1]], np.int32)
    for bad_row in (n_train, -1, 2 ** 31 - 1):
        mem = [user, np.concatenate([user[:3], [bad_row], user[3:]]), user, np.array([bad_row]), user[:1]]
        mo = np.cumsum([0] + [len(r) for r in mem]).astype(np.int64)
        G = len(mem)
        out = [torch.full((G,), 7.0, dtype=torch.float64, device=dev) for _ in range(2)]
        dth = torch.full((G * c.D,), 7.0, dtype=torch.float64, device=dev)
        ctx.group_influence(qu, qi, t([0, G], np.int64), t(mo, np.int64), t(np.concatenate(mem), np.int32),
                            out[0], out[1], dth)
        grp, fo_, dth = out[0].cpu().numpy(), out[1].cpu().numpy(), dth.cpu().numpy().reshape(G, c.D)
        for g in (1, 3):
            assert np.isnan(grp[g]) and np.isnan(fo_[g]) and np.isnan(dth[g]).all()
        for g in (0, 2):
            assert bits(grp[g:g + 1])[0] == bits(c.res["group"][a:a + 1])[0]
            assert bits(fo_[g:g + 1])[0] == bits(c.res["first_order"][a:a + 1])[0]
            assert np.array_equal(bits(dth[g]), bits(c.res["dtheta"][a]))
        assert np.isfinite(grp[4]) and np.isfinite(dth[4]).all()
    # one output at a time
    go, mo, mr = t([0, 1], np.int64), t([0, len(user)], np.int64), t(user, np.int32)
    for which in range(3):
        bufs = [torch.full((1,), 7.0, dtype=torch.float64, device=dev),
                torch.full((1,), 7.0, dtype=torch.float64, device=dev),
                torch.full((c.D,), 7.0, dtype=torch.float64, device=dev)]
        args = [bufs[j] if j == which else None for j in range(3)]
        ctx.group_influence(qu, qi, go, mo, mr, *args)
        got = bufs[which].cpu().numpy()
        assert np.array_equal(bits(got), bits(np.atleast_1d(c.res[KEYS[which]][a]))), KEYS[which]


def test_cover_independent(case):
    """After prepare_for on the queries only, the results are bitwise those after the full prepare
    (member rows name users and items outside the cover); the groups of a query outside the cover
    score NaN.  Runs last on the model."""
    c = case
    Q = len(c.qs)
    live = [q for q in range(Q) if c.cores[q]["n"]]
    import torch
    c.m.prepare_for(live)
    try:
        sub = c.m.get_group_influence(live, [c.groups[q] for q in live], return_dtheta=True)
        # a query outside the cover (user 10), through the binding: NaN, and the covered query
        # beside it keeps its bits
        ctx, dev = c.m.ctx, c.m.ctx.torch_device
        a = gid(c, 0, "user")
        user = c.flat[a]
        assert not any(u == 10 for u, _ in c.qs) and (c.tu == 10).sum() == 3
        t = lambda arr, dt: torch.from_numpy(np.ascontiguousarray(arr, dt)).to(dev)
        out = [torch.full((2,), 7.0, dtype=torch.float64, device=dev) for _ in range(2)]
        dth = torch.full((2 * c.D,), 7.0, dtype=torch.float64, device=dev)
        mem = np.concatenate([np.nonzero(c.tu == 10)[0][:1], user])
        ctx.group_influence(t([10, c.qs[0][0]], np.int32), t([2, c.qs[0][1]], np.int32), t([0, 1, 2], np.int64),
                            t([0, 1, mem.size], np.int64), t(mem, np.int32), out[0], out[1], dth)
        grp, fo_, dth = out[0].cpu().numpy(), out[1].cpu().numpy(), dth.cpu().numpy().reshape(2, c.D)
        assert np.isnan(grp[0]) and np.isnan(fo_[0]) and np.isnan(dth[0]).all()
        assert bits(grp[1:])[0] == bits(c.res["group"][a:a + 1])[0]
        assert bits(fo_[1:])[0] == bits(c.res["first_order"][a:a + 1])[0]
        assert np.array_equal(bits(dth[1]), bits(c.res["dtheta"][a]))
    finally:
        c.m.ctx.prepare()
    keep = [g for g, (q, _, _) in enumerate(c.refs) if q in live]
    for key in KEYS:
        assert np.array_equal(bits(sub[key]), bits(c.res[key][keep])), key
