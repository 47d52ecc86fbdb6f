"""GPU tests of fia_score_candidates / get_candidate_influence_batch: the influence of
hypothetical ratings (the reference's phantom-point branch, matrix_factorization.py:228-235)

    infl_c = x_q . (2 (r-hat(a, b) - y) d r-hat(a, b)/d theta_t + wd M theta_t) / n_q

against the related-rating path (a candidate equal to a related train row gets that row's
influence), against a CPU fp64 restatement of the formula built from the oracle's helpers, and
for the properties of the call: list-length edges, top-K order, independence of the
fia_prepare_for cover, the single-query API and determinism.

Tolerances are the project's: influence within RTOL = 1e-5 relative to the query's largest
|influence| (rel_err), top-K by check_topk's rule."""
import os

import numpy as np
import pytest

from influence import synth
from test_gpu_parity import RTOL, check_topk, make_model, rel_err

pytestmark = pytest.mark.gpu

WD, DAMP = 1e-3, 1e-6
U, I, N = 40, 30, 600
TILE = 256      # candidates per scoring workgroup (kCandTile, score_cand.hip)

ALL_SIZES = [("MF", 8), ("MF", 16), ("MF", 32), ("MF", 64), ("MF", 128), ("MF", 256),
             ("NCF", 8), ("NCF", 16), ("NCF", 32), ("NCF", 64), ("NCF", 128), ("NCF", 256)]


def problem(seed=0):
    """U=40, I=30, N=600; user U-1 and item I-1 have no ratings."""
    rng = np.random.default_rng(seed)
    key = np.sort(rng.choice((U - 1) * (I - 1), N, replace=False))
    tu, ti = (key // (I - 1)).astype(np.int32), (key % (I - 1)).astype(np.int32)
    tr = rng.integers(1, 6, N).astype(np.float32)
    return tu, ti, tr


def params_for(model, k, seed=3):
    return synth.mf_params(U, I, k, seed) if model == "MF" else synth.ncf_params(U, I, k, seed)


def unrated_pair(tu, ti, rng):
    while True:
        u, i = int(rng.integers(0, U - 1)), int(rng.integers(0, I - 1))
        if not ((tu == u) & (ti == i)).any():
            return u, i


def cpu_candidates(model, p, k, u, i, n, x, a, b, y):
    """The formula on the CPU in fp64: oracle._mf_core / _ncf_core's `grads @ x / n` with the
    train row replaced by the candidate (a, b, y); y as the float32 the device reads."""
    from oracle import fia_oracle as fo
    a = np.asarray(a, np.int64)
    b = np.asarray(b, np.int64)
    y = np.asarray(y, np.float32).astype(np.float64)
    is_u, is_i = a == u, b == i
    if model == "MF":
        P, Q, bu, bi, _ = fo._mf_tables(p, k)
        theta = np.concatenate([P[u], Q[i], [bu[u]], [bi[i]]])
        M = np.concatenate([np.ones(2 * k), np.zeros(2)])
        r = fo.mf_predict(p, k, a, b)
        G = np.zeros((a.size, 2 * k + 2))
        G[is_u, 0:k] = Q[b[is_u]]
        G[is_u, 2 * k] = 1.0
        G[is_i, k:2 * k] = P[a[is_i]]
        G[is_i, 2 * k + 1] = 1.0
    else:
        T = fo._ncf_tables(p, k)
        theta = np.concatenate([T["Pm"][u], T["Qm"][i], T["Pg"][u], T["Qg"][i]])
        M = np.ones(4 * k)
        r, dPm, dQm, dPg, dQg = fo.ncf_forward_backward(T, k, a, b)
        G = np.concatenate([dPm * is_u[:, None], dQm * is_i[:, None], dPg * is_u[:, None], dQg * is_i[:, None]], 1)
    e = r - y
    with np.errstate(all="ignore"):
        const = float(x @ (WD * M * theta)) / n if n else np.nan
        infl = (2.0 * e[:, None] * G + (WD * M * theta)[None, :]) @ x / n if n else np.full(a.size, np.nan)
    return infl, const


def assert_close(got, want):
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    if (~nan).any():
        assert rel_err(got[~nan], want[~nan]) < RTOL, rel_err(got[~nan], want[~nan])


# ------------------------------------------------------------------------------------------
# 1. related rows as candidates
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,k", ALL_SIZES)
def test_related_rows_as_candidates(model, k, tmp_path):
    """Every built (model, k): each query's own related rows (tu[rel], ti[rel], tr[rel]) as its
    candidates score what get_influence_batch gives those rows, and what the oracle gives.
    Queries: a pair that is itself a train row (both sides non-zero, coupled solve), a pair
    whose user has no ratings, a plain held-out pair, and one with n_q = 0, whose three
    candidates all score NaN (none is dropped)."""
    from oracle import fia_oracle as fo
    tu, ti, tr = problem()
    p = params_for(model, k)
    rng = np.random.default_rng(k)
    qs = [(int(tu[17]), int(ti[17])), (U - 1, 3), unrated_pair(tu, ti, rng), (U - 1, I - 1), (5, I - 1)]
    qu = np.array([q[0] for q in qs], np.int32)
    qi = np.array([q[1] for q in qs], np.int32)
    m = make_model(model, U, I, k, (tu, ti, tr), (qu, qi), p, wd=WD, damping=DAMP, tmpdir=tmp_path)
    ref = m.get_influence_batch(list(range(len(qs))), K=0)
    Xs, Ys, off = [], [], [0]
    for q in range(len(qs)):
        rel = ref["rel_idx"][ref["offsets"][q]:ref["offsets"][q + 1]]
        if rel.size:
            Xs.append(np.stack([tu[rel], ti[rel]], 1))
            Ys.append(tr[rel])
        else:                                   # n_q = 0: arbitrary candidates, all NaN
            Xs.append(np.array([[U - 1, I - 1], [0, 0], [U - 1, 2]], np.int32))
            Ys.append(np.array([1.5, 2.5, 3.5], np.float32))
        off.append(off[-1] + len(Ys[-1]))
    X, Y = np.concatenate(Xs), np.concatenate(Ys)
    got = m.get_candidate_influence_batch(list(range(len(qs))), np.array(off, np.int64), X, Y)
    assert got["influence"].dtype == np.float64 and got["influence"].shape == (off[-1],)
    assert np.array_equal(got["cand_offsets"], off)
    assert np.array_equal(got["x"], ref["x"], equal_nan=True)
    for q, (u, i) in enumerate(qs):
        o = fo.query(model, p, k, tu, ti, tr, u, i, WD, DAMP)
        mine = got["influence"][off[q]:off[q + 1]]
        if o["n"] == 0:
            assert mine.size == 3 and np.isnan(mine).all()
            continue
        theirs = ref["influence"][ref["offsets"][q]:ref["offsets"][q + 1]]
        print("%s k=%d q=%d n=%d: vs related path %.2e, vs oracle %.2e" % (
            model, k, q, o["n"], rel_err(mine, theirs), rel_err(mine, o["influence"])))
        assert rel_err(mine, theirs) < RTOL, (model, k, q)
        assert rel_err(mine, o["influence"]) < RTOL, (model, k, q)
    m.ctx.close()


# ------------------------------------------------------------------------------------------
# 2. arbitrary candidates against the CPU formula, x given
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,k", [(mo, k) for mo in ("MF", "NCF") for k in (8, 16, 64, 256)])
def test_arbitrary_candidates_match_cpu_formula(model, k, tmp_path):
    """x given as the oracle's x.  Per query: same user with an item the user never rated, same
    item with a new user, (u, i) itself at y in {1.0, 2.5, 5.0}, a pair sharing neither (which
    scores the constant x . (wd M theta_t) / n_q), and one exact duplicate.  The other ratings
    are non-integer, so nothing passes by e = 0."""
    from oracle import fia_oracle as fo
    tu, ti, tr = problem()
    p = params_for(model, k)
    rng = np.random.default_rng(100 + k)
    qs = [(int(tu[17]), int(ti[17])), (U - 1, 3), unrated_pair(tu, ti, rng), (7, I - 1)]
    qu = np.array([q[0] for q in qs], np.int32)
    qi = np.array([q[1] for q in qs], np.int32)
    m = make_model(model, U, I, k, (tu, ti, tr), (qu, qi), p, wd=WD, damping=DAMP, tmpdir=tmp_path)
    orc = [fo.query(model, p, k, tu, ti, tr, u, i, WD, DAMP) for u, i in qs]
    xs = np.stack([o["x"] for o in orc])
    Xs, Ys, off = [], [], [0]
    for u, i in qs:
        b_new = next(b for b in range(I) if b != i and not ((tu == u) & (ti == b)).any())
        a_new = next(a for a in range(U) if a != u and not ((tu == a) & (ti == i)).any())
        a_far, b_far = (u + 3) % U, (i + 4) % I
        c = [(u, b_new, 3.3), (a_new, i, 1.7), (u, i, 1.0), (u, i, 2.5), (u, i, 5.0), (a_far, b_far, 4.2),
             (u, b_new, 3.3)]
        Xs.append(np.array([(a, b) for a, b, _ in c], np.int64))
        Ys.append(np.array([y for _, _, y in c], np.float64))
        off.append(off[-1] + len(c))
    X, Y = np.concatenate(Xs), np.concatenate(Ys)
    got = m.get_candidate_influence_batch(list(range(len(qs))), np.array(off, np.int64), X, Y, inverse_hvp=xs)
    assert np.array_equal(got["x"], xs)
    for q, (u, i) in enumerate(qs):
        b, e = off[q], off[q + 1]
        want, const = cpu_candidates(model, p, k, u, i, orc[q]["n"], xs[q], X[b:e, 0], X[b:e, 1], Y[b:e])
        mine = got["influence"][b:e]
        print("%s k=%d q=%d: rel err %.2e, constant %.3e vs %.3e" % (model, k, q, rel_err(mine, want), mine[5], const))
        assert rel_err(mine, want) < RTOL, (model, k, q)
        assert abs(mine[5] - const) <= RTOL * abs(const), (model, k, q)       # shares neither: the constant
        assert mine[6] == mine[0]                                             # exact duplicate: same bits
    m.ctx.close()


# ------------------------------------------------------------------------------------------
# 3, 4, 7: one batch of list-length edges per model, shared
# ------------------------------------------------------------------------------------------
COUNTS = [0, 1, 63, 64, 65, 255, 256, 257, 1025, 62, 256, 512, 257, 511, 513, 0]
DUP_LIST, DUP_LO, DUP_HI = 8, 300, 700      # the 1025-candidate list holds one duplicated outlier


@pytest.fixture(scope="module", params=["MF", "NCF"])
def edges(request, tmp_path_factory):
    from oracle import fia_oracle as fo
    model, k = request.param, 16
    tu, ti, tr = problem()
    p = params_for(model, k)
    rng = np.random.default_rng(7)
    pairs = [(int(tu[17]), int(ti[17])), (U - 1, 3), unrated_pair(tu, ti, rng), (7, I - 1), (U - 1, I - 1)]
    qs = [pairs[j % 4] for j in range(len(COUNTS))]
    qs[4] = pairs[4]                            # the 65-candidate list belongs to a query with n_q = 0
    qu = np.array([q[0] for q in qs], np.int32)
    qi = np.array([q[1] for q in qs], np.int32)
    m = make_model(model, U, I, k, (tu, ti, tr), (qu, qi), p, wd=WD, damping=DAMP,
                   tmpdir=tmp_path_factory.mktemp("edges_" + model))
    off = np.concatenate([[0], np.cumsum(COUNTS)]).astype(np.int64)
    M = int(off[-1])
    X = np.stack([rng.integers(0, U, M), rng.integers(0, I, M)], 1).astype(np.int64)
    Y = (rng.random(M) * 4.0 + 1.0).astype(np.float32)
    share = rng.integers(0, 4, M)               # 0: as drawn, 1: the query's user, 2: its item, 3: both
    for q, (u, i) in enumerate(qs):
        sl = slice(off[q], off[q + 1])
        X[sl, 0] = np.where(share[sl] & 1, u, X[sl, 0])
        X[sl, 1] = np.where(share[sl] & 2, i, X[sl, 1])
    u8, i8 = qs[DUP_LIST]
    for pos in (DUP_LO, DUP_HI):                # (u, i) at y = 1000: by far the largest |influence|
        X[off[DUP_LIST] + pos] = (u8, i8)
        Y[off[DUP_LIST] + pos] = 1000.0
    Q = len(qs)
    full = m.get_candidate_influence_batch(list(range(Q)), off, X, Y, K=0)
    want = np.empty(M)
    for q, (u, i) in enumerate(qs):
        n = int((tu == u).sum() + (ti == i).sum())
        b, e = off[q], off[q + 1]
        want[b:e] = cpu_candidates(model, p, k, u, i, n, full["x"][q], X[b:e, 0], X[b:e, 1], Y[b:e])[0]
    yield dict(model=model, m=m, qs=qs, off=off, X=X, Y=Y, full=full, want=want)
    m.ctx.close()


def test_list_length_edges(edges):
    """Candidate counts 0, 1, 63, 64, 65, 255, 256, 257 and 1025 in one batch, an empty list
    first and another last.  The scoring kernel's one work-item length is its tile of 256
    consecutive candidates of the WHOLE batch (kCandTile), so the edges that matter are
    where the lists fall on the tile grid: the first tile holds five whole lists and the head of
    a sixth (several segments per tile); the 62-candidate list ends at 2048, so the following
    256- and 512-candidate lists cover exactly one and exactly two tiles; 257 then overhangs a
    tile by one; 511 starts one past the grid and ends exactly on it (3584); 513 starts on the
    grid and overhangs two tiles by one.  The 65-candidate list
    belongs to a query with n_q = 0 (all NaN).  Against the CPU formula with the call's own x."""
    off = edges["off"]
    assert off[10] % TILE == 0 and off[11] % TILE == 0 and off[12] % TILE == 0 and off[14] % TILE == 0
    got = edges["full"]["influence"]
    assert got.shape == (off[-1],)
    for q in range(len(COUNTS)):
        b, e = off[q], off[q + 1]
        if q == 4:
            assert np.isnan(got[b:e]).all()
        else:
            assert np.isfinite(got[b:e]).all()
        assert_close(got[b:e], edges["want"][b:e])


@pytest.mark.parametrize("K", [1, 4, 64])
def test_topk(edges, K):
    """Top-K of every list of the edge batch: selection bit-exact on the kernel's own values,
    -1 / NaN padding where the list is shorter than K, the duplicated outlier resolved to its
    lower position, topk_val the bits of influence[pos]; with influence = NULL (full=False) and
    K = 4 the same top-K bit for bit."""
    m, off, X, Y = edges["m"], edges["off"], edges["X"], edges["Y"]
    Q = len(COUNTS)
    infl = edges["full"]["influence"]
    res = m.get_candidate_influence_batch(list(range(Q)), off, X, Y, K=K)
    assert np.array_equal(res["influence"].view(np.int64), infl.view(np.int64))
    assert res["topk_pos"].shape == (Q, K) and res["topk_pos"].dtype == np.int64
    for q in range(Q):
        b, e = off[q], off[q + 1]
        pos, val = res["topk_pos"][q], res["topk_val"][q]
        if q == 4:      # all NaN: positions in order
            assert np.array_equal(pos[:min(K, 65)], np.arange(min(K, 65))) and np.isnan(val).all()
            continue
        check_topk(pos, infl[b:e], edges["want"][b:e], K)
        nsel = min(K, e - b)
        assert (pos[nsel:] == -1).all() and np.isnan(val[nsel:]).all()
        assert np.array_equal(val[:nsel].view(np.int64), infl[b:e][pos[:nsel]].view(np.int64))
    assert res["topk_pos"][DUP_LIST][0] == DUP_LO
    if K > 1:
        assert res["topk_pos"][DUP_LIST][1] == DUP_HI
        assert res["topk_val"][DUP_LIST][0] == res["topk_val"][DUP_LIST][1]
    if K == 4:
        lean = m.get_candidate_influence_batch(list(range(Q)), off, X, Y, K=K, full=False)
        assert "influence" not in lean
        assert np.array_equal(lean["topk_pos"], res["topk_pos"])
        assert np.array_equal(lean["topk_val"].view(np.int64), res["topk_val"].view(np.int64))


def test_deterministic(edges):
    m, off, X, Y = edges["m"], edges["off"], edges["X"], edges["Y"]
    Q = len(COUNTS)
    a = m.get_candidate_influence_batch(list(range(Q)), off, X, Y, K=4)
    b = m.get_candidate_influence_batch(list(range(Q)), off, X, Y, K=4)
    for key in ("influence", "x", "topk_val"):
        assert np.array_equal(a[key].view(np.int64), b[key].view(np.int64)), key
    assert np.array_equal(a["topk_pos"], b["topk_pos"])
    assert np.array_equal(a["influence"].view(np.int64), edges["full"]["influence"].view(np.int64))


def test_batch_limit_is_refused_before_launch(edges):
    """total_cand above FIA_CAND_MAX_TOTAL (2^31 - 1): FIA_ERR_INVALID from the argument checks,
    before anything is reserved or launched (the arrays passed are never read)."""
    import torch
    m = edges["m"]
    dev = m.ctx.torch_device
    q = torch.zeros(1, dtype=torch.int32, device=dev)
    x = torch.zeros(m.ctx.num_params(), dtype=torch.float64, device=dev)
    off = torch.zeros(2, dtype=torch.int64, device=dev)
    f = torch.zeros(1, dtype=torch.float32, device=dev)
    ptr = lambda t: t.data_ptr()
    rc = m.ctx.lib.fia_score_candidates(m.ctx.h, 1, ptr(q), ptr(q), ptr(x), ptr(off), 2 ** 31, ptr(q), ptr(q), ptr(f),
                                        None, 0, None, None, None)
    assert rc == 1
    rc = m.ctx.lib.fia_score_candidates(m.ctx.h, 1, ptr(q), ptr(q), ptr(x), ptr(off), 0, None, None, None,
                                        None, 4, None, None, None)
    assert rc == 1          # K > 0 with null top-K outputs
    rc = m.ctx.lib.fia_score_candidates(m.ctx.h, 0, None, None, None, None, 0, None, None, None, None, 0, None, None,
                                        None)
    assert rc == 0          # no queries: nothing to do


# ------------------------------------------------------------------------------------------
# 5. independence of the fia_prepare_for cover
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,k", [("MF", 16), ("NCF", 16), ("NCF", 64)])
def test_cover_independence(model, k, tmp_path):
    """After prepare_for(subset) candidates whose other entity lies outside the subset's users
    and items score bit for bit what they score after a full prepare."""
    tu, ti, tr = problem()
    p = params_for(model, k)
    qs = [(int(tu[17]), int(ti[17])), (2, 9), (11, 4)]
    qu = np.array([q[0] for q in qs], np.int32)
    qi = np.array([q[1] for q in qs], np.int32)
    m = make_model(model, U, I, k, (tu, ti, tr), (qu, qi), p, wd=WD, damping=DAMP, tmpdir=tmp_path)
    out_u = [a for a in range(U) if a not in qu][:6]
    out_i = [b for b in range(I) if b not in qi][:6]
    Xs, Ys, off = [], [], [0]
    for u, i in qs:
        c = [(u, b) for b in out_i] + [(a, i) for a in out_u] + [(a, b) for a, b in zip(out_u, out_i)] + [(u, i)]
        Xs.append(np.array(c, np.int64))
        Ys.append(np.linspace(1.25, 4.75, len(c)))
        off.append(off[-1] + len(c))
    X, Y, off = np.concatenate(Xs), np.concatenate(Ys), np.array(off, np.int64)
    full = m.get_candidate_influence_batch([0, 1, 2], off, X, Y, K=3)
    m.prepare_for([0, 1, 2])
    part = m.get_candidate_influence_batch([0, 1, 2], off, X, Y, K=3)
    assert np.isfinite(full["influence"]).all()
    for key in ("influence", "x", "topk_val"):
        assert np.array_equal(part[key].view(np.int64), full[key].view(np.int64)), key
    assert np.array_equal(part["topk_pos"], full["topk_pos"])
    m.ctx.close()


# ------------------------------------------------------------------------------------------
# 6. the single-query API
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["MF", "NCF"])
def test_single_query_phantom_points(model, tmp_path):
    """get_influence_on_test_loss([t], None, X=X, Y=Y) returns the batch call's influence bit
    for bit and sets train_indices_of_test_case as the normal call does; with
    force_refresh=False and a cached flat inverse-HVP file it scores with that vector."""
    k = 16
    tu, ti, tr = problem()
    p = params_for(model, k)
    qs = [(int(tu[17]), int(ti[17])), (2, 9)]
    qu = np.array([q[0] for q in qs], np.int32)
    qi = np.array([q[1] for q in qs], np.int32)
    m = make_model(model, U, I, k, (tu, ti, tr), (qu, qi), p, wd=WD, damping=DAMP, tmpdir=tmp_path)
    rng = np.random.default_rng(3)
    for t, (u, i) in enumerate(qs):
        X = np.stack([rng.integers(0, U, 40), rng.integers(0, I, 40)], 1)
        X[:10, 0] = u
        X[5:15, 1] = i
        Y = rng.random(40) * 4.0 + 1.0
        normal = m.get_influence_on_test_loss([t], np.arange(N))
        rel = m.train_indices_of_test_case.copy()
        x0 = np.concatenate([np.ravel(a) for a in m.inverse_hvp])
        one = m.get_influence_on_test_loss([t], None, X=X, Y=Y)
        assert one.dtype == np.float64 and one.shape == (40,) and normal.shape == rel.shape
        assert np.array_equal(m.train_indices_of_test_case, rel)
        assert m.test_index == t and (m.test_u, m.test_i) == (u, i) and m.num_params == x0.size
        assert np.array_equal(np.concatenate([np.ravel(a) for a in m.inverse_hvp]), x0)
        batch = m.get_candidate_influence_batch([t], np.array([0, 40], np.int64), X, Y)
        assert np.array_equal(one.view(np.int64), batch["influence"].view(np.int64))
        # the cache file the first call wrote, doubled: scored with that vector (influence is
        # linear in x, a power-of-two scale is exact)
        fname = os.path.join(str(tmp_path), "test_%s-cg-normal_loss-test-[%d].npz" % (model, t))
        assert os.path.exists(fname)
        np.savez(fname, inverse_hvp=2.0 * x0)
        twice = m.get_influence_on_test_loss([t], None, X=X, Y=Y, force_refresh=False)
        given = m.get_candidate_influence_batch([t], np.array([0, 40], np.int64), X, Y, inverse_hvp=2.0 * x0)
        assert np.array_equal(twice.view(np.int64), given["influence"].view(np.int64))
        assert np.array_equal(twice, 2.0 * one)
    m.ctx.close()
