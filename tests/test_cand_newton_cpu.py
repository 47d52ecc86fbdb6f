"""CPU tests of the Newton-corrected candidate call: fia_score_candidates_newton is declared,
exported and bound and refuses a NULL context; the facade validates on the host -- ValueError
before any GPU call (the objects here have no GPU context); and the numpy reference the GPU tests
compare against, cand_newton_reference, whose two routes must agree:

  * the definition of include/fia.h, one np.linalg.solve per candidate:
        H_c = (1/n) (2 g_c g_c^T + 2 e_c C [both] + wd diag(M)),  b_c = (1/n) (2 e_c g_c + wd M theta)
        newton_add = v . (H + H_c)^-1 b_c
  * the closed form for every candidate that is not `both`:
        H" = H + (wd/n) diag(M), c = 2/n, x" = H"^-1 v, w" = H"^-1 (wd M theta)/n, c" = x" . (wd M theta)/n
        s = x" . g, t = w" . g, h = g^T H"^-1 g
        newton_add = 2 e s / n + c" - c s (2 e h / n + t) / (1 + c h)

The inputs are an oracle.fia_oracle.query core and the candidates' gradients, built as
cpu_candidates of tests/test_gpu_candidates.py builds them; C as in group_reference.  The problem
and the queries are those of tests/test_newton_cpu.py; candidate_lists builds the batch that
tests/test_gpu_cand_newton.py runs."""
import ctypes

import numpy as np
import pytest

from influence import _lib, synth
from influence.NCF import NCF
from influence.matrix_factorization import MF
from oracle import fia_oracle as fo

from test_abi import header_functions
from test_group_cpu import w3g_of
from test_newton_cpu import DAMP, DUP, I, U, WD, _one_blas_thread, problem, queries

SIZES = [("MF", 8), ("MF", 16), ("MF", 32), ("MF", 64), ("NCF", 8), ("NCF", 16), ("NCF", 32)]
COND_MAX = 1e8
CLOSED_TOL = 1e-9           # of the query's largest |value| (measured worst 5.8e-11)


def params_for(model, k):
    return synth.mf_params(U, I, k, 3) if model == "MF" else synth.ncf_params(U, I, k, 3)


def candidate_gradients(model, p, k, u, i, a, b, y):
    """Per candidate (a, b, y) of query (u, i), ids in range: G [m, D] = d r-hat(a, b) / d theta_t in
    the reference theta order with the blocks of a side that does not match the query zeroed,
    e [m] = r-hat(a, b) - y (y as the float32 the device reads) and both [m]."""
    a = np.asarray(a, np.int64)
    b = np.asarray(b, np.int64)
    y = np.asarray(y, np.float32).astype(np.float64)
    is_u, is_i = a == u, b == i
    if model == "MF":
        P, Q, _, _, _ = fo._mf_tables(p, k)
        r = fo.mf_predict(p, k, a, b)
        G = np.zeros((a.size, 2 * k + 2))
        G[is_u, 0:k] = Q[b[is_u]]
        G[is_u, 2 * k] = 1.0
        G[is_i, k:2 * k] = P[a[is_i]]
        G[is_i, 2 * k + 1] = 1.0
    else:
        T = fo._ncf_tables(p, k)
        r, dPm, dQm, dPg, dQg = fo.ncf_forward_backward(T, k, a, b)
        G = np.concatenate([dPm * is_u[:, None], dQm * is_i[:, None], dPg * is_u[:, None], dQg * is_i[:, None]], 1)
    return G, r - y, is_u & is_i


def cand_newton_reference(core, G, e, both, wd, W3g=None):
    """Per candidate of an oracle query with n > 0: dict(newton [m] by the definition, closed [m] by
    the closed form (NaN at `both` candidates), first [m] the first-order x . b_c, cond [m] of
    H + H_c, cpp = c", min_den the smallest |1 + c h| met and its most negative value neg_den)."""
    n, v, H, theta, x = core["n"], core["v"], core["H"], core["theta"], core["x"]
    D = theta.size
    ncf = W3g is not None
    k = D // 4 if ncf else (D - 2) // 2
    M = np.ones(D) if ncf else np.concatenate([np.ones(2 * k), np.zeros(2)])
    C = np.zeros((D, D))                                # d2 r-hat / d theta_u d theta_i, both orders
    idx = np.arange(k)
    if ncf:
        C[2 * k + idx, 3 * k + idx] = C[3 * k + idx, 2 * k + idx] = W3g
    else:
        C[idx, k + idx] = C[k + idx, idx] = 1.0
    m = e.size
    rhs = wd * M * theta / n
    newton, cond, first = np.zeros(m), np.zeros(m), np.zeros(m)
    with _one_blas_thread():
        for j in range(m):
            Hc = (2.0 * np.outer(G[j], G[j]) + (2.0 * e[j] * C if both[j] else 0.0) + np.diag(wd * M)) / n
            bc = 2.0 * e[j] * G[j] / n + rhs
            newton[j] = v @ np.linalg.solve(H + Hc, bc)
            cond[j] = np.linalg.cond(H + Hc)
            first[j] = x @ bc
        Hpp = H + np.diag(wd * M) / n
        xpp, wpp = np.linalg.solve(Hpp, v), np.linalg.solve(Hpp, rhs)
        PG = np.linalg.solve(Hpp, G.T).T if m else np.zeros((0, D))
    cpp, c = float(xpp @ rhs), 2.0 / n
    s, t, h = G @ xpp, G @ wpp, np.einsum("pd,pd->p", G, PG)
    den = 1.0 + c * h
    closed = 2.0 * e * s / n + cpp - c * s * (2.0 * e * h / n + t) / den
    closed[both] = np.nan
    live = ~both
    return dict(newton=newton, closed=closed, first=first, cond=cond, cpp=cpp,
                min_den=float(np.abs(den[live]).min()) if live.any() else np.inf,
                neg_den=float(den[live].min()) if live.any() else np.inf)


def candidate_lists(tu, ti, qs):
    """The candidate batch of tests/test_gpu_cand_newton.py for the queries of test_newton_cpu:
    (offsets int64 [Q + 1], users, items int64 [M], ratings float32 [M], dup = the two positions of
    query 0's list that hold the same (a, b, y)).  Ratings are non-integer, so nothing passes by
    e = 0.
      query 0 (0, i0): 300 user-side candidates (0, b), b = 0 .. 299 -- the segment crosses a
        256-position wave tile and leaves a tile tail of 12; b = i0 is a `both` candidate -- with the
        item-side candidates (a, i0), a = 0 .. 16, at every 18th position (a = 0: `both` again, with
        another y), three candidates sharing neither side, the bad ids a = U and b = -1, and the
        candidate of position 1 once more at the end (more than 300 positions on)
      the duplicated pair: a `both` candidate and 15 user-side ones; (0, 318): 16 user-side and one
        item-side; (19, i0): 17 user-side (a user with no ratings); the non-train pair: `both`, 64
        item-side -- user 19, who has no ratings, among them; (19, 319), n_q = 0: four candidates;
        (18, 300): 65 user-side; (18, 301): none; then short mixed lists."""
    rng = np.random.default_rng(71)
    i0 = qs[0][1]
    assert qs[0] == (0, i0) and qs[1] == DUP and qs[5] == (19, 319) and qs[-1] == qs[0]
    lists = []
    side_u = [(0, b) for b in range(300)]
    side_i = [(a, i0) for a in range(17)]
    first = []
    for pos in range(317):
        first.append(side_i[pos // 18] if pos % 18 == 0 and pos // 18 < 17 else side_u[pos - min(pos // 18 + 1, 17)])
    assert first[0] == (0, i0) and first[18] == (1, i0) and first[288] == (16, i0) and first[-1] == (0, 299)
    assert len(set(first)) == 316                       # (0, i0) is there from both sides
    first += [(5, 11), (18, 310), (19, 0), (U, 3), (0, -1)]
    lists.append(first)
    lists.append([DUP] + [(DUP[0], b) for b in range(100, 115)])
    lists.append([(0, b) for b in range(20, 36)] + [(7, 318)])
    lists.append([(19, b) for b in range(18) if b != i0])
    u4, i4 = qs[4]
    others = [a for a in range(U) if a != u4]
    lists.append([(u4, i4)] + [(others[j % len(others)], i4) for j in range(64)])
    assert (19, i4) in lists[-1]
    lists.append([(19, 319), (0, 0), (19, 2), (3, 319)])
    lists.append([(18, b) for b in range(65)])
    lists.append([])
    lists.append([(19, 7), (2, 301), (4, 9)])
    lists.append([(1, 1), (2, 2)])
    lists.append([(18, 299), (18, 5), (0, 299), (6, 6), (18, 299)])
    lists.append([(0, 17), (4, i0), (9, 9)])
    assert len(lists) == len(qs)
    X = np.array([c for l in lists for c in l], np.int64).reshape(-1, 2)
    Y = (rng.random(X.shape[0]) * 4.0 + 1.0).astype(np.float32)
    off = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int64)
    # the duplicate: position 1 of query 0's list once more, behind everything else of the list
    X = np.insert(X, off[1], X[1], axis=0)
    Y = np.insert(Y, off[1], Y[1])
    off[1:] += 1
    dup = (1, int(off[1]) - 1)
    assert dup[1] - dup[0] >= 300 and tuple(X[dup[0]]) == tuple(X[dup[1]]) and Y[dup[0]] == Y[dup[1]]
    return off, X[:, 0].copy(), X[:, 1].copy(), Y, dup


def test_candidate_lists_hold_what_the_gpu_test_needs():
    tu, ti, _ = problem()
    qs = queries(tu, ti)
    off, cu, ci, _, _ = candidate_lists(tu, ti, qs)
    lens = np.diff(off)
    assert lens[0] == 323 and lens[7] == 0 and off[-1] == cu.size
    seg = {}                                            # (query, side) -> candidates
    both = 0
    for q, (u, i) in enumerate(qs):
        a, b = cu[off[q]:off[q + 1]], ci[off[q]:off[q + 1]]
        ok = (a >= 0) & (a < U) & (b >= 0) & (b < I)
        both += int((ok & (a == u) & (b == i)).sum())
        seg[(q, 0)] = int((ok & (a == u) & (b != i)).sum())
        seg[(q, 1)] = int((ok & (a != u) & (b == i)).sum())
    assert seg[(0, 0)] == 300 and seg[(0, 1)] == 16     # (0, 0) is listed twice; b = i0 and a = 0 are `both`
    assert {1, 15, 16, 17, 64, 65} <= set(seg.values())
    assert both >= 4


@pytest.mark.parametrize("model,k", SIZES)
def test_closed_form_is_the_definition(model, k):
    """Every live query of the problem with 24 random candidates: user side, item side, both,
    neither, in equal shares."""
    tu, ti, tr = problem()
    p = params_for(model, k)
    W3g = w3g_of(model, p, k)
    rng = np.random.default_rng(1000 + k)
    worst, worst_cond, neg_den, seen_both = 0.0, 0.0, np.inf, 0
    for (u, i) in queries(tu, ti)[:-1]:
        core = fo.query(model, p, k, tu, ti, tr, u, i, WD, DAMP)
        if not core["n"]:
            continue
        a, b = rng.integers(0, U, 24), rng.integers(0, I, 24)
        share = np.arange(24) % 4                       # 0: as drawn, 1: the user, 2: the item, 3: both
        a, b = np.where(share & 1, u, a), np.where(share & 2, i, b)
        y = rng.random(24) * 4.0 + 1.0
        G, e, both = candidate_gradients(model, p, k, u, i, a, b, y)
        ref = cand_newton_reference(core, G, e, both, WD, W3g)
        assert ref["cond"].max() < COND_MAX, ((u, i), ref["cond"].max())
        live = ~both
        seen_both += int(both.sum())
        scale = np.abs(ref["newton"]).max()
        err = np.abs(ref["closed"][live] - ref["newton"][live]).max() / scale
        worst, worst_cond, neg_den = max(worst, err), max(worst_cond, ref["cond"].max()), min(neg_den, ref["neg_den"])
        assert err < CLOSED_TOL, ((u, i), err)
        neither = (a != u) & (b != i)
        assert np.abs(ref["newton"][neither] - ref["cpp"]).max() < CLOSED_TOL * scale
    assert seen_both >= 6 * 10
    print("%s k=%d: closed form within %.2e, largest cond(H + H_c) %.3e, smallest 1 + c h %.3e" % (
        model, k, worst, worst_cond, neg_den))


def test_score_candidates_newton_declared_exported_bound(libfia_path):
    assert "fia_score_candidates_newton" in header_functions()
    assert hasattr(ctypes.CDLL(libfia_path), "fia_score_candidates_newton")
    assert "fia_score_candidates_newton" in _lib.SIGNATURES
    lib = _lib.load_library(libfia_path)
    rc = lib.fia_score_candidates_newton(None, 0, None, None, None, 0, None, None, None, None, 0, None, None, None)
    assert rc == 1
    assert lib.fia_version() == 100


@pytest.mark.parametrize("cls", [MF, NCF])
def test_candidate_newton_host_validation(cls):
    m = cls.__new__(cls)          # no GPU context: only the host-side validation is exercised
    m.num_users, m.num_items, m.embedding_size, m.num_train_examples = 7, 5, 8, 20
    X = np.array([[0, 0], [1, 1], [2, 2]])
    Y = np.array([1.0, 2.0, 3.0])
    off = np.array([0, 2, 3])
    for kwargs in (dict(K=-1), dict(K=_lib.FIA_MAX_TOPK + 1), dict(K=1.5), dict(K=True), dict(K=0, full=False)):
        with pytest.raises(ValueError):
            m.get_candidate_newton_batch([0, 1], off, X, Y, **kwargs)
    bad = [(np.array([0, 2]), X, Y),                    # Q + 1 offsets
           (np.array([0, 3, 2]), X, Y),                 # decreasing
           (np.array([1, 2, 3]), X, Y),                 # does not start at 0
           (np.array([0, 2, 4]), X, Y),                 # does not end at len(Y)
           (off, X[:, :1], Y),                          # X not [M, 2]
           (off, X, Y[:2]),                             # lengths differ
           (off, np.array([[0, 0], [7, 1], [2, 2]]), Y),        # user id out of range
           (off, np.array([[0, 0], [1, -1], [2, 2]]), Y),       # item id out of range
           (off, np.array([[0, 0], [1.5, 1], [2, 2]]), Y)]      # not an integer id
    for o, x, y in bad:
        with pytest.raises(ValueError):
            m.get_candidate_newton_batch([0, 1], o, x, y, K=1)
