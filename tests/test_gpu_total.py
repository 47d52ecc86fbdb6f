"""GPU tests of fia_total_influence / get_total_influence: for every train row the sum of its
influence on a batch of predictions,

    total[j] = sum_q m_q(j) x_q . (2 e_j g_j + wd M theta_t(q)) / n_q,   count[j] = sum_q m_q(j)

with m_q(j) how often row j occurs in q's related list -- the scatter-add by rel_idx of the
per-query influences.  The reference is that scatter-add (np.add.at) of the fp64 oracle's
per-query influences, and of get_influence_batch's own output; count is np.bincount(rel_idx)
exactly.

Tolerance: the project's, rel_err(total, want) < RTOL = 1e-5 relative to the largest |want|
(the oracle-side reordering of the sum costs ~1e-15); top-K selection bit-exact on the call's
own total."""
import numpy as np
import pytest

from influence import synth
from influence.dataset import DataSet
from test_gpu_candidates import ALL_SIZES, I, N, U, params_for, problem, unrated_pair
from test_gpu_parity import RTOL, make_model, rel_err

pytestmark = pytest.mark.gpu

WD, DAMP = 1e-3, 1e-6
TILE = 256      # list positions per train-row workgroup (kTotalTile, total.hip)


class Oracle(object):
    """fo.query per DISTINCT pair, cached; scatter-adds of its per-query influences."""

    def __init__(self, model, p, k, tu, ti, tr):
        self.args = (model, p, k, tu, ti, tr)
        self.n_train = len(tr)
        self.cache = {}

    def query(self, u, i):
        from oracle import fia_oracle as fo
        if (u, i) not in self.cache:
            self.cache[(u, i)] = fo.query(*self.args, u, i, WD, DAMP)
        return self.cache[(u, i)]

    def xs(self, qs):
        return np.stack([self.query(u, i)["x"] for u, i in qs])

    def total(self, qs, weights=None):
        total = np.zeros(self.n_train)
        count = np.zeros(self.n_train, np.int64)
        for q, (u, i) in enumerate(qs):
            o = self.query(u, i)
            if o["n"] == 0:
                continue
            np.add.at(total, o["rel"], o["influence"] * (1.0 if weights is None else weights[q]))
            np.add.at(count, o["rel"], 1)
        return total, count


def model_for(model, k, train, qs, p, tmpdir, U_=U, I_=I, labels=None):
    qu = np.array([q[0] for q in qs], np.int32)
    qi = np.array([q[1] for q in qs], np.int32)
    m = make_model(model, U_, I_, k, train, (qu, qi), p, wd=WD, damping=DAMP, tmpdir=tmpdir)
    if labels is not None:
        m.data_sets["test"] = DataSet(np.stack([qu, qi], 1), np.asarray(labels, np.float64))
    return m


def check_total(res, want, want_count):
    got, cnt = res["total"], res["count"]
    assert got.dtype == np.float64 and cnt.dtype == np.int32 and got.shape == want.shape == cnt.shape
    assert np.array_equal(cnt, want_count)
    assert np.isfinite(got).all()
    err = rel_err(got, want)
    print("rel err %.2e (largest |want| %.3e)" % (err, np.abs(want).max(initial=0.0)))
    assert err < RTOL, err
    untouched = cnt == 0
    assert (got[untouched].view(np.int64) == 0).all()          # exactly +0.0


def small_queries(tu, ti, seed):
    """~40 queries on the U=40, I=30, N=600 problem: a pair that is a train row, the same pair
    again, one sharing only its user, one sharing only its item, a user with no ratings, (U-1, I-1)
    with n_q = 0, random pairs (rated or not) for the rest."""
    rng = np.random.default_rng(seed)
    u0, i0 = int(tu[17]), int(ti[17])
    only_u = next(b for b in range(I - 1) if not ((tu == u0) & (ti == b)).any())
    only_i = next(a for a in range(U - 1) if not ((tu == a) & (ti == i0)).any())
    qs = [(u0, i0), (u0, i0), (u0, only_u), (only_i, i0), (U - 1, 3), (U - 1, I - 1), unrated_pair(tu, ti, rng)]
    while len(qs) < 40:
        qs.append((int(rng.integers(0, U - 1)), int(rng.integers(0, I - 1))))
    return qs


# ------------------------------------------------------------------------------------------
# 1. every built (model, k), x from the solve
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,k", ALL_SIZES)
def test_total_matches_scatter_add(model, k, tmp_path):
    tu, ti, tr = problem()
    p = params_for(model, k)
    qs = small_queries(tu, ti, k)
    m = model_for(model, k, (tu, ti, tr), qs, p, tmp_path)
    orc = Oracle(model, p, k, tu, ti, tr)
    want, want_count = orc.total(qs)
    res = m.get_total_influence(list(range(len(qs))))
    assert np.isnan(res["x"][5]).all()                          # n_q = 0: TF's mean over an empty batch
    check_total(res, want, want_count)
    # the route it replaces: the batch call's own per-rating output, scatter-added by rel_idx
    ref = m.get_influence_batch(list(range(len(qs))), K=0)
    mine = np.zeros(N)
    np.add.at(mine, ref["rel_idx"], ref["influence"])
    assert np.array_equal(res["count"], np.bincount(ref["rel_idx"], minlength=N))
    assert rel_err(res["total"], mine) < RTOL
    m.ctx.close()


# ------------------------------------------------------------------------------------------
# 2. x given: the new kernels without the solve
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,k", [(mo, k) for mo in ("MF", "NCF") for k in (8, 64)])
def test_total_with_given_x(model, k, tmp_path):
    tu, ti, tr = problem()
    p = params_for(model, k)
    qs = small_queries(tu, ti, 50 + k)
    m = model_for(model, k, (tu, ti, tr), qs, p, tmp_path)
    orc = Oracle(model, p, k, tu, ti, tr)
    xs = orc.xs(qs)
    assert np.isnan(xs[5]).all()
    res = m.get_total_influence(list(range(len(qs))), inverse_hvp=xs)
    assert np.array_equal(res["x"], xs, equal_nan=True)
    check_total(res, *orc.total(qs))
    m.ctx.close()


# ------------------------------------------------------------------------------------------
# 3, 4, 5: the edge problem and batch, per model and train size, shared
# ------------------------------------------------------------------------------------------
U2, I2 = 12, 560
LONG = 2 * TILE + 7             # user 0's list: longer than two train-row tiles
DUP_A, DUP_B = (3, 5), (4, 6)   # train pairs present in two rows: A with equal ratings, B with different ones


def edge_problem(n_drop):
    """User 0 has LONG ratings (list positions [0, LONG)), user 1's list ends exactly on the tile
    boundary 3 TILE, users 2 and 11 have none; users 3 .. 10 have 32 each (users 7 .. 10 on items
    no query names: their rows stay untouched), (3, 5) and (4, 6) are present twice.  Rows are
    shuffled, so a train row is not its list position.  N = 4 TILE; n_drop > 0 drops rows of
    user 10 (the last list) so that N is no multiple of the tile."""
    rng = np.random.default_rng(11)
    rows = [(0, b, 0.0) for b in range(LONG)] + [(1, b, 0.0) for b in range(3 * TILE - LONG)]
    per = (4 * TILE - 3 * TILE) // 8       # 32 rows for each of users 3 .. 10
    for a in range(3, 11):
        lo, hi = (60, 100) if a < 7 else (100, I2 - 1)
        items = list(rng.choice(np.arange(lo, hi), per - (2 if a in (3, 4) else 0), replace=False))
        if a == 3:
            items += [DUP_A[1], DUP_A[1]]
        if a == 4:
            items += [DUP_B[1], DUP_B[1]]
        rows += [(a, int(b), 0.0) for b in items]
    assert len(rows) == 4 * TILE
    tu = np.array([r[0] for r in rows], np.int32)
    ti = np.array([r[1] for r in rows], np.int32)
    tr = (rng.random(len(rows)) * 4.0 + 1.0).astype(np.float32)
    tr[(tu == DUP_A[0]) & (ti == DUP_A[1])] = 2.75              # equal ratings: equal totals
    perm = rng.permutation(len(rows))
    # the dropped rows are user 10's (the last list): every other list keeps its place
    last = np.nonzero(tu == 10)[0][:n_drop]
    perm = np.array([j for j in perm if j not in set(last.tolist())])
    tu, ti, tr = tu[perm], ti[perm], tr[perm]
    # list positions (user-major): the properties the kernel's tiles see
    deg = np.bincount(tu, minlength=U2)
    ends = np.cumsum(deg)
    assert deg[0] > 2 * TILE and ends[1] % TILE == 0 and deg[2] == 0 and deg[11] == 0
    assert ((tu == DUP_A[0]) & (ti == DUP_A[1])).sum() == 2 and ((tu == DUP_B[0]) & (ti == DUP_B[1])).sum() == 2
    assert (len(tr) % TILE == 0) == (n_drop == 0)
    return tu, ti, tr


def edge_queries():
    """Query groups per entity of sizes 0, 1, 63, 64, 65 and 257: user 0 has 257 queries (64 on
    item 10, 65 on item 11, 63 on item 12, 65 over items 13 .. 39: 30 distinct pairs, most of
    them train rows), user 1 has 65, user 3 has 64 (DUP_A once), user 4 has 63 (DUP_B twice),
    user 5 one, user 2 (no ratings) one, and (11, I2 - 1) has n_q = 0; users 6 .. 10 have none."""
    qs = [(0, 10)] * 64 + [(0, 11)] * 65 + [(0, 12)] * 63 + [(0, 13 + t % 27) for t in range(65)]
    qs += [(1, 40 + t % 10) for t in range(65)]
    qs += [DUP_A] + [(3, 60 + t % 9) for t in range(63)]
    qs += [DUP_B, DUP_B] + [(4, 70 + t % 7) for t in range(61)]
    qs += [(5, 80), (2, 3), (11, I2 - 1)]
    rng = np.random.default_rng(5)
    order = rng.permutation(len(qs))                     # groups are not contiguous in the batch
    qs = [qs[j] for j in order]
    cu = np.bincount([q[0] for q in qs], minlength=U2)
    ci = np.bincount([q[1] for q in qs], minlength=I2)
    assert list(cu[:7]) == [257, 65, 1, 64, 63, 1, 0] and (ci[10], ci[11], ci[12]) == (64, 65, 63)
    assert len(set(q for q in qs if q[0] == 0)) <= 30
    return qs


@pytest.fixture(scope="module", params=[("MF", 0), ("NCF", 0), ("MF", 3), ("NCF", 3)],
                ids=lambda v: "%s-drop%d" % v)
def edges(request, tmp_path_factory):
    model, n_drop = request.param
    k = 16
    tu, ti, tr = edge_problem(n_drop)
    p = synth.mf_params(U2, I2, k, 3) if model == "MF" else synth.ncf_params(U2, I2, k, 3)
    qs = edge_queries()
    rng = np.random.default_rng(9)
    labels = rng.random(len(qs)) * 4.0 + 1.0
    m = model_for(model, k, (tu, ti, tr), qs, p, tmp_path_factory.mktemp("total_%s%d" % (model, n_drop)),
                  U_=U2, I_=I2, labels=labels)
    orc = Oracle(model, p, k, tu, ti, tr)
    want, want_count = orc.total(qs)
    res = m.get_total_influence(list(range(len(qs))))
    yield dict(model=model, k=k, m=m, qs=qs, train=(tu, ti, tr), p=p, orc=orc, want=want, want_count=want_count,
               res=res, labels=labels)
    m.ctx.close()


def test_edges_match_oracle(edges):
    """Lists longer than two tiles, ending on a tile boundary and empty; query groups of 0, 1,
    63, 64, 65 and 257; duplicated train pairs queried once and twice; N a multiple of the tile
    and not.  Rows whose user and item have no query: +0.0 and count 0 (check_total)."""
    tu, ti, tr = edges["train"]
    res = edges["res"]
    check_total(res, edges["want"], edges["want_count"])
    assert (res["count"] == 0).sum() >= 3 * 32                   # users 7 .. 10 (minus the dropped rows)
    for (a, b), times in ((DUP_A, 1), (DUP_B, 2)):
        rows = np.nonzero((tu == a) & (ti == b))[0]
        assert rows.size == 2
        # each of the pair's queries holds both rows twice; every other query of the user or
        # the item once
        others_u = sum(1 for q in edges["qs"] if q[0] == a) - times
        others_i = sum(1 for q in edges["qs"] if q[1] == b) - times
        assert (res["count"][rows] == 2 * times + others_u + others_i).all()
    ra = np.nonzero((tu == DUP_A[0]) & (ti == DUP_A[1]))[0]
    assert res["total"][ra[0]] == res["total"][ra[1]]            # equal ratings: the same bits


def want_topk(total, count, K):
    rows = np.nonzero(count > 0)[0]
    order = rows[np.lexsort((rows, -np.abs(total[rows])))][:K]
    return order


@pytest.mark.parametrize("K", [1, 4, 64])
def test_topk(edges, K):
    """The K rows of largest |total| among the touched rows: bit-exact on the call's own total,
    ties to the lower train row; full=False gives the same bits."""
    m, Q = edges["m"], len(edges["qs"])
    full = edges["res"]
    res = m.get_total_influence(list(range(Q)), K=K)
    assert np.array_equal(res["total"].view(np.int64), full["total"].view(np.int64))
    assert np.array_equal(res["count"], full["count"])
    assert res["topk_idx"].shape == (K,) and res["topk_idx"].dtype == np.int64
    want = want_topk(full["total"], full["count"], K)
    assert want.size == K
    assert np.array_equal(res["topk_idx"], want)
    assert np.array_equal(res["topk_val"].view(np.int64), full["total"][want].view(np.int64))
    lean = m.get_total_influence(list(range(Q)), K=K, full=False)
    assert "total" not in lean and "count" not in lean
    assert np.array_equal(lean["topk_idx"], res["topk_idx"])
    assert np.array_equal(lean["topk_val"].view(np.int64), res["topk_val"].view(np.int64))


def test_topk_padding_and_tie(edges):
    """A batch of one query, DUP_A, with n_q < 64: its touched rows, all of them, then -1 / NaN;
    the two rows of the pair have equal totals (equal ratings) and come lower row first."""
    m, qs = edges["m"], edges["qs"]
    tu, ti, tr = edges["train"]
    t = qs.index(DUP_A)
    n_q = int((tu == DUP_A[0]).sum() + (ti == DUP_A[1]).sum())
    assert 2 < n_q < 64
    res = m.get_total_influence([t], K=64)
    touched = n_q - 2                                            # the pair's two rows are in both lists
    assert (res["count"] > 0).sum() == touched
    want = want_topk(res["total"], res["count"], 64)
    assert want.size == touched
    assert np.array_equal(res["topk_idx"][:touched], want)
    assert (res["topk_idx"][touched:] == -1).all() and np.isnan(res["topk_val"][touched:]).all()
    assert np.array_equal(res["topk_val"][:touched].view(np.int64), res["total"][want].view(np.int64))
    ra = np.nonzero((tu == DUP_A[0]) & (ti == DUP_A[1]))[0]
    pos = [int(np.nonzero(res["topk_idx"] == r)[0][0]) for r in ra]
    assert pos[1] == pos[0] + 1 and res["topk_val"][pos[0]] == res["topk_val"][pos[1]]
    assert (res["count"][ra] == 2).all()
    o = edges["orc"].query(*DUP_A)
    want_total = np.zeros(len(tr))
    np.add.at(want_total, o["rel"], o["influence"])
    assert rel_err(res["total"], want_total) < RTOL


def test_weights(edges):
    """weights = 2 everywhere: exactly 2 * total (a power of two commutes with every rounding);
    a weight of 0 on one query equals dropping it; get_influence_on_test_set_loss is the call
    with weights 2 (r-hat_q - y_q) / Q."""
    from oracle import fia_oracle as fo
    m, qs, Q = edges["m"], edges["qs"], len(edges["qs"])
    full = edges["res"]
    twice = m.get_total_influence(list(range(Q)), weights=np.full(Q, 2.0), inverse_hvp=full["x"])
    same = m.get_total_influence(list(range(Q)), inverse_hvp=full["x"])
    assert np.array_equal(same["total"].view(np.int64), full["total"].view(np.int64))
    assert np.array_equal(twice["total"], 2.0 * full["total"])
    assert np.array_equal(twice["x"], full["x"], equal_nan=True)          # x is returned unscaled
    assert np.array_equal(twice["count"], full["count"])
    t = qs.index((5, 80))
    w = np.ones(Q)
    w[t] = 0.0
    zeroed = m.get_total_influence(list(range(Q)), weights=w, inverse_hvp=full["x"])
    keep = [q for q in range(Q) if q != t]
    dropped = m.get_total_influence(keep, inverse_hvp=full["x"][keep])
    assert rel_err(zeroed["total"], dropped["total"]) < RTOL
    want, _ = edges["orc"].total([qs[q] for q in keep])
    assert rel_err(zeroed["total"], want) < RTOL
    # the test-set loss
    qu = np.array([q[0] for q in qs])
    qi = np.array([q[1] for q in qs])
    pred = (fo.mf_predict if edges["model"] == "MF" else fo.ncf_predict)(edges["p"], edges["k"], qu, qi)
    wl = 2.0 * (pred - edges["labels"]) / Q
    loss = m.get_influence_on_test_set_loss(list(range(Q)), K=4)
    assert rel_err(loss["weights"], wl) < RTOL
    mine = m.get_total_influence(list(range(Q)), weights=wl, K=4)
    assert rel_err(loss["total"], mine["total"]) < RTOL
    assert np.array_equal(loss["count"], mine["count"])
    want, _ = edges["orc"].total(qs, weights=wl)
    assert rel_err(loss["total"], want) < RTOL
    assert np.array_equal(loss["topk_idx"], want_topk(loss["total"], loss["count"], 4))


def test_raw_abi(edges):
    """Q = 0 zeroes the outputs and returns 0; no output at all, or K > 0 without top-K arrays,
    returns 1; Q = 2^30 + 1 returns 1 from the argument checks (the arrays are never read)."""
    import torch
    m = edges["m"]
    dev = m.ctx.torch_device
    n = m.ctx.n_train
    lib, h = m.ctx.lib, m.ctx.h
    ptr = lambda t: t.data_ptr()
    total = torch.full((n,), 7.0, dtype=torch.float64, device=dev)
    count = torch.full((n,), 7, dtype=torch.int32, device=dev)
    ti = torch.full((4,), 7, dtype=torch.int64, device=dev)
    tv = torch.full((4,), 7.0, dtype=torch.float64, device=dev)
    assert lib.fia_total_influence(h, 0, None, None, None, ptr(total), ptr(count), 4, ptr(ti), ptr(tv), None) == 0
    torch.cuda.synchronize()
    assert (total.cpu().numpy().view(np.int64) == 0).all() and (count.cpu().numpy() == 0).all()
    assert (ti.cpu().numpy() == -1).all() and np.isnan(tv.cpu().numpy()).all()
    q = torch.zeros(1, dtype=torch.int32, device=dev)
    x = torch.zeros(m.ctx.num_params(), dtype=torch.float64, device=dev)
    assert lib.fia_total_influence(h, 1, ptr(q), ptr(q), ptr(x), None, None, 0, None, None, None) == 1
    assert lib.fia_total_influence(h, 1, ptr(q), ptr(q), ptr(x), ptr(total), None, 4, None, None, None) == 1
    assert lib.fia_total_influence(h, 2 ** 30 + 1, ptr(q), ptr(q), ptr(x), ptr(total), ptr(count), 0, None, None,
                                   None) == 1
    assert lib.fia_total_influence(h, 1, ptr(q), ptr(q), ptr(x), ptr(total), ptr(count), 65, ptr(ti), ptr(tv),
                                   None) == 1


# ------------------------------------------------------------------------------------------
# 6. determinism and independence of the fia_prepare_for cover
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,k", [("MF", 16), ("NCF", 16), ("NCF", 64)])
def test_deterministic_and_cover_independent(model, k, tmp_path):
    """Two calls give the same bits; after prepare_for(a subset of the queries) the call with
    the same inverse_hvp gives the bits it gave after the full prepare."""
    tu, ti, tr = problem()
    p = params_for(model, k)
    qs = small_queries(tu, ti, 7)
    Q = len(qs)
    m = model_for(model, k, (tu, ti, tr), qs, p, tmp_path)
    a = m.get_total_influence(list(range(Q)), K=8)
    b = m.get_total_influence(list(range(Q)), K=8, inverse_hvp=a["x"])
    for key in ("total", "topk_val"):
        assert np.array_equal(a[key].view(np.int64), b[key].view(np.int64)), key
    assert np.array_equal(a["count"], b["count"]) and np.array_equal(a["topk_idx"], b["topk_idx"])
    m.prepare_for([0, 2, 3])
    c = m.get_total_influence(list(range(Q)), K=8, inverse_hvp=a["x"])
    for key in ("total", "topk_val"):
        assert np.array_equal(a[key].view(np.int64), c[key].view(np.int64)), key
    assert np.array_equal(a["count"], c["count"]) and np.array_equal(a["topk_idx"], c["topk_idx"])
    m.ctx.close()
