"""CPU tests of the slate call: fia_count_related_slate and fia_slate_batch are declared, exported and
bound and refuse a NULL context; the facade validates on the host -- ValueError before any GPU call
(the objects here have no GPU context); and the numpy reference the GPU tests compare against,
slate_reference, the definition of include/fia.h stated row by row over the related list:

    theta_t = (theta_u, theta_i1 .. theta_im),  rel = R_u ++ C_i1 ++ .. ++ C_im,  n = |rel|
    H = (2/n) sum_p (g_p g_p^T + e_p d2 r-hat_p) + wd diag(M) + damping I
    v = d (sum_l w_l r-hat(u, i_l)) / d theta_t,  x = H^-1 v  (one np.linalg.solve)
    influence_p = x . (2 e_p g_p + wd M theta_t) / n,  value = sum_l w_l r-hat(u, i_l)

in the extended reference theta order (MF [p_u, q_1 .. q_m, b_u, b_1 .. b_m], NCF [Pm_u, Qm_1 ..,
Pg_u, Qg_1 ..]).  It is checked against pair_reference (m = 2, w = (1, -1)), against the oracle's
single query (m = 1), against a torch double-backward over the m + 1 slices, and against the route
the kernel takes -- the arrowhead solved block by block with an LDL^T per block and no full-matrix
solve (slate_route).  The problem is that of tests/test_newton_cpu.py; slate_list builds the batch
that tests/test_gpu_slate.py runs, and every slate of it is asserted here to give cond(H) < 1e8."""
import ctypes
import types

import numpy as np
import pytest

from influence import _lib
from influence.NCF import NCF
from influence.matrix_factorization import MF
from oracle import fia_oracle as fo

from test_abi import header_functions
from test_cand_newton_cpu import COND_MAX, params_for
from test_newton_cpu import DAMP, DUP, I, U, WD, _one_blas_thread, problem, queries
from test_pair_cpu import SIZES as PAIR_SIZES, pair_list, pair_reference

SIZES = [("MF", 8), ("MF", 16), ("MF", 32), ("MF", 64), ("NCF", 8), ("NCF", 16), ("NCF", 32)]


def disc(m):
    """The facade's default weights: DCG's discount 1 / log2(rank + 2), rank from 0."""
    return (1.0 / np.log2(np.arange(m) + 2.0)).tolist()


def slate_blocks(model, k, m):
    """Index arrays of the user block and the m item blocks in the extended reference theta order."""
    idx = np.arange(k)
    if model == "MF":
        return [np.concatenate([b * k + idx, [(m + 1) * k + b]]) for b in range(m + 1)]
    return [np.concatenate([b * k + idx, (m + 1) * k + b * k + idx]) for b in range(m + 1)]


def slate_model(model, p, k, u, items):
    """(theta_t, M, predict(a, b), gradient(a, b) [D_q], blocks, E) of the slate (u; items): the
    gradient of r-hat(a, b) in theta_t has its user block zero unless a == u and its block l unless
    b == i_l; d2 r-hat / d theta_t^2 of the own pair (u, i_l) is diag(E) on the (block l, user block)
    cross blocks."""
    idx = np.arange(k)
    m = len(items)
    blocks = slate_blocks(model, k, m)
    where = {int(b): l for l, b in enumerate(items)}
    if model == "MF":
        P, Q, bu, bi, g = fo._mf_tables(p, k)
        Dq = (m + 1) * (k + 1)
        theta = np.zeros(Dq)
        theta[blocks[0]] = np.concatenate([P[u], [bu[u]]])
        for l, b in enumerate(items):
            theta[blocks[1 + l]] = np.concatenate([Q[b], [bi[b]]])
        M = np.concatenate([np.ones((m + 1) * k), np.zeros(m + 1)])

        def predict(a, b):
            return float(P[a] @ Q[b] + bu[a] + bi[b] + g)

        def gradient(a, b):
            G = np.zeros(Dq)
            if a == u:
                G[blocks[0]] = np.concatenate([Q[b], [1.0]])
            if b in where:
                G[blocks[1 + where[b]]] = np.concatenate([P[a], [1.0]])
            return G
        E = np.concatenate([np.ones(k), [0.0]])
    else:
        T = fo._ncf_tables(p, k)
        Dq = (m + 1) * 2 * k
        theta = np.zeros(Dq)
        theta[blocks[0]] = np.concatenate([T["Pm"][u], T["Pg"][u]])
        for l, b in enumerate(items):
            theta[blocks[1 + l]] = np.concatenate([T["Qm"][b], T["Qg"][b]])
        M = np.ones(Dq)

        def predict(a, b):
            return float(fo.ncf_forward_backward(T, k, [a], [b])[0][0])

        def gradient(a, b):
            _, dPm, dQm, dPg, dQg = fo.ncf_forward_backward(T, k, [a], [b])
            G = np.zeros(Dq)
            if a == u:
                G[blocks[0]] = np.concatenate([dPm[0], dPg[0]])
            if b in where:
                G[blocks[1 + where[b]]] = np.concatenate([dQm[0], dQg[0]])
            return G
        E = np.concatenate([np.zeros(k), T["W3"][k // 2:]])
    return theta, M, predict, gradient, blocks, E


def slate_rel(tu, ti, u, items):
    return np.concatenate([np.nonzero(tu == u)[0]] + [np.nonzero(ti == b)[0] for b in items]).astype(np.int64)


def slate_reference(model, p, k, tu, ti, tr, u, items, w, wd, damping):
    """The definition in numpy, row by row over rel, with one np.linalg.solve.  Returns dict(rel, n,
    H, v, x, influence, value, cond, theta, G [n, D_q], e [n]); n = 0 gives NaN H / x / cond and no
    influence."""
    tu, ti = np.asarray(tu), np.asarray(ti)
    items = [int(b) for b in items]
    w = np.asarray(w, np.float64)
    assert len(set(items)) == len(items) == w.size >= 1
    y = np.asarray(tr, np.float32).astype(np.float64)
    rel = slate_rel(tu, ti, u, items)
    n = rel.size
    theta, M, predict, gradient, blocks, E = slate_model(model, p, k, u, items)
    Dq = theta.size
    v = sum(w[l] * gradient(u, b) for l, b in enumerate(items))
    value = float(sum(w[l] * predict(u, b) for l, b in enumerate(items)))
    if n == 0:
        return dict(rel=rel, n=0, H=np.full((Dq, Dq), np.nan), v=v, x=np.full(Dq, np.nan), influence=np.zeros(0),
                    value=value, cond=np.nan, theta=theta, G=np.zeros((0, Dq)), e=np.zeros(0))
    G, e = np.zeros((n, Dq)), np.zeros(n)
    own = np.zeros((Dq, Dq))                           # sum_p e_p d2 r-hat_p: own-pair rows only
    for pos, row in enumerate(rel):
        a, b = int(tu[row]), int(ti[row])
        e[pos] = predict(a, b) - y[row]
        G[pos] = gradient(a, b)
        if a == u and b in items:
            bl = blocks[1 + items.index(b)]
            own[bl, blocks[0]] += e[pos] * E
            own[blocks[0], bl] += e[pos] * E
    H = (2.0 / n) * (G.T @ G + own) + np.diag(wd * M + damping)     # sum_p g_p g_p^T = G^T G
    with _one_blas_thread():
        x = np.linalg.solve(H, v)
        cond = float(np.linalg.cond(H))
    infl = (2.0 * e[:, None] * G + (wd * M * theta)[None, :]) @ x / n
    return dict(rel=rel, n=n, H=H, v=v, x=x, influence=infl, value=value, cond=cond, theta=theta, G=G, e=e)


def slate_list(tu, ti):
    """The thirteen slates (user, items, weights) of tests/test_gpu_slate.py, the table of the call's
    issue; i4 and i5 as in pair_list."""
    pl = pair_list(tu, ti)
    i4, i5 = pl[3][1], pl[3][2]
    return [
        (0, [7, 8], [1.0, -1.0]),
        (DUP[0], [i4], [1.0]),
        (0, [7, 318, 8, 299, 40, 12], disc(6)),
        (DUP[0], [DUP[1], i4, i5], [1.0, 0.5, -0.25]),
        (19, [7, 300, 301, 302], disc(4)),
        (18, [300, 301, 302, 1, 2, 299, 310], disc(7)),
        (1, list(range(16)), disc(16)),
        (0, list(range(32)), disc(32)),
        (0, [7, 8, 9], [1.0, 0.0, 0.5]),
        (18, [299], [1.0]),
        (17, [302, 301, 5], [0.2, 0.3, 0.5]),
        (19, [318, 319], [1.0, 1.0]),
        (0, [7, 8], [1.0, -1.0]),
    ]


MAX_ITEMS = _lib.FIA_SLATE_MAX_ITEMS
LONG = (0, list(range(MAX_ITEMS)), disc(MAX_ITEMS))       # the maximal length, every item rated by the user


def coupled_count(tu, ti, u, items):
    return sum(int(((tu == u) & (ti == b)).any()) for b in items)


# ------------------------------------------------------------------------------------------
# the reference against the existing references
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,k", PAIR_SIZES)
def test_two_items_are_the_pair(model, k):
    """m = 2, w = (1, -1): pair_reference's system -- H, v, x, the influences and the gap within
    1e-12 of the largest value."""
    tu, ti, tr = problem()
    p = params_for(model, k)
    i4 = pair_list(tu, ti)[3][1]
    for (u, i, j) in ((0, 7, 8), (DUP[0], DUP[1], i4)):
        ref = slate_reference(model, p, k, tu, ti, tr, u, [i, j], [1.0, -1.0], WD, DAMP)
        pr = pair_reference(model, p, k, tu, ti, tr, u, i, j, WD, DAMP)
        assert np.array_equal(ref["rel"], pr["rel"])
        for key in ("H", "v", "x", "influence"):
            err = np.abs(ref[key] - pr[key]).max() / np.abs(pr[key]).max()
            print("%s k=%d (%d, %d, %d) %s: %.2e" % (model, k, u, i, j, key, err))
            assert err < 1e-12, (key, err)
        assert abs(ref["value"] - pr["diff"]) <= 1e-12 * max(1.0, abs(pr["diff"]))


@pytest.mark.parametrize("model,k", SIZES)
def test_one_item_is_the_single_query(model, k):
    """m = 1, w = (1): the oracle's query -- rel, x and the influences within 1e-12."""
    tu, ti, tr = problem()
    p = params_for(model, k)
    for (u, i) in queries(tu, ti)[:5] + [(18, 299)]:
        ref = slate_reference(model, p, k, tu, ti, tr, u, [i], [1.0], WD, DAMP)
        one = fo.query(model, p, k, tu, ti, np.asarray(tr, np.float32).astype(np.float64), u, i, WD, DAMP)
        assert np.array_equal(ref["rel"], one["rel"])
        for key in ("x", "influence"):
            err = np.abs(ref[key] - one[key]).max() / np.abs(one[key]).max()
            assert err < 1e-12, ((u, i), key, err)


def autograd_slate(model, p, k, tu, ti, tr, u, items, w, wd, damping):
    """H, v and the influences of the slate system by torch double backward over the m + 1 slices,
    built as test_pair_cpu.autograd_pair is."""
    import torch
    from oracle import autograd_oracle as ao
    build = ao._mf_graph if model == "MF" else ao._ncf_graph
    plist, logits, decayed = build(p, k, U, I)
    if model == "MF":
        sl = [(0, u * k, k)] + [(1, b * k, k) for b in items] + [(2, u, 1)] + [(3, b, 1) for b in items]
    else:
        sl = ([(0, u * k, k)] + [(1, b * k, k) for b in items] + [(2, u * k, k)] + [(3, b * k, k) for b in items])
    Dq = sum(s[2] for s in sl)
    rel = slate_rel(tu, ti, u, items)
    n = rel.size
    users = torch.tensor(tu[rel], dtype=torch.long)
    its = torch.tensor(ti[rel], dtype=torch.long)
    y = torch.tensor(np.asarray(tr, np.float32).astype(np.float64)[rel])

    def total_loss(us, bs, ys):
        return ((logits(us, bs) - ys) ** 2).mean() + sum(0.5 * (q ** 2).sum() for q in decayed) * wd

    def sliced(grads):
        grads = [torch.zeros_like(q) if g is None else g for q, g in zip(plist, grads)]
        return torch.cat([grads[pi].reshape(-1)[s:s + L] for pi, s, L in sl])

    f = (logits(torch.tensor([u] * len(items)), torch.tensor(items)) * torch.tensor(w, dtype=torch.float64)).sum()
    v = sliced(torch.autograd.grad(f, plist, allow_unused=True)).detach().numpy()
    g1s = sliced(torch.autograd.grad(total_loss(users, its, y), plist, create_graph=True))
    H = np.zeros((Dq, Dq))
    for c in range(Dq):
        unit = torch.zeros(Dq, dtype=torch.float64)
        unit[c] = 1.0
        H[:, c] = sliced(torch.autograd.grad((g1s * unit).sum(), plist, retain_graph=True,
                                             allow_unused=True)).detach().numpy()
    H += damping * np.eye(Dq)
    x = np.linalg.solve(H, v)
    infl = np.zeros(n)
    for r in range(n):
        gr = sliced(torch.autograd.grad(total_loss(users[r:r + 1], its[r:r + 1], y[r:r + 1]), plist,
                                        allow_unused=True)).detach().numpy()
        infl[r] = x @ gr / n
    return dict(H=H, v=v, influence=infl)


@pytest.mark.parametrize("model,k", [("MF", 8), ("NCF", 8)])
def test_reference_against_autograd(model, k):
    """S2 (five coupled items and an empty list) and S4 (the empty user, block diagonal): H, v and
    the influences within 1e-10 of the largest entry."""
    tu, ti, tr = problem()
    p = params_for(model, k)
    slates = slate_list(tu, ti)
    for s in (2, 4):
        u, items, w = slates[s]
        ref = slate_reference(model, p, k, tu, ti, tr, u, items, w, WD, DAMP)
        ag = autograd_slate(model, p, k, tu, ti, tr, u, items, w, WD, DAMP)
        for key in ("H", "v", "influence"):
            err = np.abs(ref[key] - ag[key]).max() / np.abs(ag[key]).max()
            print("%s k=%d S%d %s: %.2e" % (model, k, s, key, err))
            assert err < 1e-10, (s, key, err)


# ------------------------------------------------------------------------------------------
# the route of the kernel
# ------------------------------------------------------------------------------------------
def ldlt(A):
    """Unpivoted LDL^T of a symmetric matrix (nothing assumed about a pivot's sign): (L, d)."""
    n = A.shape[0]
    L, d = np.eye(n), np.zeros(n)
    for j in range(n):
        d[j] = A[j, j] - (L[j, :j] ** 2) @ d[:j]
        L[j + 1:, j] = (A[j + 1:, j] - (L[j + 1:, :j] * L[j, :j]) @ d[:j]) / d[j]
    return L, d


def ldlt_apply(L, d, b):
    """(L D L^T)^-1 b by the substitutions alone."""
    n = d.size
    y = np.array(b, np.float64)
    for j in range(n):
        y[j + 1:] -= L[j + 1:, j] * y[j]
    y /= d
    for j in range(n - 1, -1, -1):
        y[:j] -= L[j, :j] * y[j]
    return y


def slate_route(model, p, k, tu, ti, tr, u, items, w, wd, damping):
    """x by the route of slate.hip: the arrowhead block by block from the entity Grams and the pair
    terms (cd, es) -- an LDL^T per item block, the rated items' Schur complements taken out of the
    user block, its LDL^T, the rated items' back-substitution.  No matrix larger than Ds x Ds."""
    y = np.asarray(tr, np.float32).astype(np.float64)
    m = len(items)
    theta, M, predict, gradient, blocks, E = slate_model(model, p, k, u, items)
    bu = blocks[0]
    Ds = bu.size
    n = slate_rel(tu, ti, u, items).size
    diag = wd * M[bu] + damping                        # (the same in every block)

    def gram(rows, blk):
        S = np.zeros((Ds, Ds))
        for row in rows:
            g = gradient(int(tu[row]), int(ti[row]))[blk]
            S += np.outer(g, g)
        return S
    s2n, alpha = 2.0 / n, 4.0 / n
    S = s2n * gram(np.nonzero(tu == u)[0], bu) + np.diag(diag)
    r = np.zeros(Ds)
    x = np.zeros(theta.size)
    info = []
    for l, b in enumerate(items):
        bl = blocks[1 + l]
        vv = gradient(u, b)
        vu, vl = vv[bu], vv[bl]
        own = np.nonzero((tu == u) & (ti == b))[0]
        cd = float(own.size)
        es = cd * predict(u, b) - y[own].sum()
        Hll = s2n * (gram(np.nonzero(ti == b)[0], bl) + cd * np.outer(vl, vl)) + np.diag(diag)
        L, d = ldlt(Hll)
        pv = ldlt_apply(L, d, vl)
        r += w[l] * vu
        info.append((cd, es, L, d, pv, vu))
        if cd == 0:
            x[bl] = w[l] * pv
            continue
        S += s2n * cd * np.outer(vu, vu)
        dot = vl @ pv
        Epv = E * pv
        S -= alpha ** 2 * (cd * cd * dot * np.outer(vu, vu) + cd * es * (np.outer(vu, Epv) + np.outer(Epv, vu)))
        for c in np.nonzero(E)[0]:
            t = ldlt_apply(L, d, np.eye(Ds)[c])
            S[:, c] -= alpha ** 2 * es * es * E * E[c] * t
        r -= alpha * w[l] * (cd * dot * vu + es * Epv)
    L, d = ldlt(S)
    xu = ldlt_apply(L, d, r)
    x[bu] = xu
    for l, (cd, es, L, d, pv, vu) in enumerate(info):
        if cd > 0:
            x[blocks[1 + l]] = w[l] * pv - alpha * cd * (vu @ xu) * pv - alpha * es * ldlt_apply(L, d, E * xu)
    return x


@pytest.mark.parametrize("model,k", SIZES)
def test_route_and_conditioning(model, k):
    """Every slate of the GPU test's batch, and the 64-item one: cond(H) < 1e8, none skipped, and
    the block-by-block route gives the reference's x within 1e-11 of max|x|."""
    tu, ti, tr = problem()
    p = params_for(model, k)
    worst_cond, worst_route = 0.0, 0.0
    for s, (u, items, w) in enumerate(slate_list(tu, ti)[:-1] + [LONG]):
        ref = slate_reference(model, p, k, tu, ti, tr, u, items, w, WD, DAMP)
        if not ref["n"]:
            assert (u, items) == (19, [318, 319]) and np.isfinite(ref["value"])
            continue
        assert np.isfinite(ref["x"]).all()
        assert ref["cond"] < COND_MAX, (s, ref["cond"])
        worst_cond = max(worst_cond, ref["cond"])
        xr = slate_route(model, p, k, tu, ti, tr, u, items, w, WD, DAMP)
        err = np.abs(xr - ref["x"]).max() / np.abs(ref["x"]).max()
        worst_route = max(worst_route, err)
        assert err < 1e-11, (s, err)
    print("%s k=%d: largest cond(H) %.3e, route against the full solve %.2e" % (model, k, worst_cond, worst_route))


def test_slate_list_holds_what_the_gpu_test_needs():
    tu, ti, tr = problem()
    sl = slate_list(tu, ti)
    n = lambda u, items: int((tu == u).sum() + sum((ti == b).sum() for b in items))
    assert len(sl) == 13 and sl[0] == sl[12] and sl[0][:2] == (0, [7, 8])
    assert all(len(set(items)) == len(items) == len(w) and 1 <= len(items) <= _lib.FIA_SLATE_MAX_ITEMS
               for (_, items, w) in sl + [LONG])
    assert [len(items) for (_, items, _) in sl] == [2, 1, 6, 3, 4, 7, 16, 32, 3, 1, 3, 2, 2]
    assert [coupled_count(tu, ti, u, items) for (u, items, _) in sl] == [2, 0, 5, 1, 0, 3, 13, 32, 3, 0, 1, 0, 2]
    assert coupled_count(tu, ti, *LONG[:2]) == 64 and len(LONG[1]) == _lib.FIA_SLATE_MAX_ITEMS
    assert ((tu == DUP[0]) & (ti == DUP[1])).sum() == 2 and sl[3][0] == DUP[0] and sl[3][1][0] == DUP[1]
    assert (tu == 0).sum() == 300 and (ti == 318).sum() == 0 and (tu == 19).sum() == 0
    assert [int((ti == b).sum()) for b in (300, 301, 302, 299, 40, 310)] == [15, 16, 17, 1, 1, 1]
    assert n(*sl[2][:2]) == 334 and n(*sl[7][:2]) == 619 and n(*sl[9][:2]) == 4 and n(*sl[11][:2]) == 0
    assert n(*sl[0][:2]) > 256                           # the first query's list crosses a scoring tile
    # S6: coupled and uncoupled items interleaved
    own6 = [bool(((tu == 1) & (ti == b)).any()) for b in sl[6][1]]
    assert 0 < own6.index(False) < 15 and True in own6[own6.index(False):]
    assert sl[8][2][1] == 0.0                            # a zero weight


def test_not_the_weighted_sum_of_singles():
    """S2 on user 0's list, MF k=16: the slate values are not the weighted sum of the six single
    queries' (the issue's table gives 2.3 times the largest slate value)."""
    tu, ti, tr = problem()
    p = params_for("MF", 16)
    u, items, w = slate_list(tu, ti)[2]
    ref = slate_reference("MF", p, 16, tu, ti, tr, u, items, w, WD, DAMP)
    du = int((tu == u).sum())
    y = np.asarray(tr, np.float32).astype(np.float64)
    singles = sum(w[l] * fo.query("MF", p, 16, tu, ti, y, u, b, WD, DAMP)["influence"][:du]
                  for l, b in enumerate(items))
    gap = np.abs(ref["influence"][:du] - singles).max() / np.abs(ref["influence"]).max()
    print("largest |slate - weighted singles| / largest |slate| on the user's list: %.3e" % gap)
    assert gap > 1e-3


# ------------------------------------------------------------------------------------------
# ABI and facade
# ------------------------------------------------------------------------------------------
def test_slate_calls_declared_exported_bound(libfia_path):
    for name in ("fia_count_related_slate", "fia_slate_batch"):
        assert name in header_functions()
        assert hasattr(ctypes.CDLL(libfia_path), name)
        assert name in _lib.SIGNATURES
    lib = _lib.load_library(libfia_path)
    assert lib.fia_count_related_slate(None, 0, None, None, 0, None, None, None, None) == 1
    assert lib.fia_slate_batch(None, 0, None, None, 0, None, None, None, 0, None, None, None, None, 0, None, None,
                               None, None) == 1
    assert lib.fia_version() == 100


@pytest.mark.parametrize("cls", [MF, NCF])
def test_slate_batch_host_validation(cls):
    m = cls.__new__(cls)          # no GPU context: only the host-side validation is exercised
    m.num_users, m.num_items, m.embedding_size, m.num_train_examples = 7, 5, 8, 20
    good_u, good_s = [0, 3], [[1, 2], [4]]
    for users, slates in (([0], good_s), ([0, 3, 4], good_s),          # a length mismatch
                          ([0.5, 3.0], good_s), ([[0, 3]], good_s),    # users: not integers, not 1-d
                          ([-1, 3], good_s), ([0, 7], good_s),         # a user out of range
                          (good_u, [[1, 2.5], [4]]),                   # items: not integers
                          (good_u, [[1, -1], [4]]), (good_u, [[1, 5], [4]]),   # an item out of range
                          (good_u, [[1, 2], []]),                      # m = 0
                          (good_u, [[1, 1], [4]]),                     # a repeated item
                          (good_u, [[[1, 2]], [4]])):                  # not 1-d
        with pytest.raises(ValueError):
            m.get_slate_influence_batch(users, slates, K=1)
    m.num_items = 100
    with pytest.raises(ValueError):
        m.get_slate_influence_batch([0], [list(range(_lib.FIA_SLATE_MAX_ITEMS + 1))], K=1)       # m = 65
    m.num_items = 5
    for weights in ([[1.0, 2.0]], [[1.0], [1.0]], [[1.0, np.nan], [1.0]], [[1.0, np.inf], [1.0]],
                    [[1.0, "a"], [1.0]], [[1.0, 2.0, 3.0], [1.0]]):
        with pytest.raises(ValueError):
            m.get_slate_influence_batch(good_u, good_s, weights=weights, K=1)
    for K in (-1, _lib.FIA_MAX_TOPK + 1, 1.5, True):
        with pytest.raises(ValueError):
            m.get_slate_influence_batch(good_u, good_s, K=K)
    u, soff, items, wts = m._checked_slates(good_u, good_s, None)
    assert u.dtype == np.int32 and items.dtype == np.int32 and soff.tolist() == [0, 2, 3] and items.tolist() == [1, 2, 4]
    assert wts.dtype == np.float64 and np.array_equal(wts, np.array(disc(2) + disc(1)))
    assert m._checked_slates(good_u, good_s, [[1.0, 0.0], [-2]])[3].tolist() == [1.0, 0.0, -2.0]
