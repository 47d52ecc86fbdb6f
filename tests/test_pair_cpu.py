"""CPU tests of the pair call: fia_count_related_pair and fia_pair_batch are declared, exported and
bound and refuse a NULL context; the facade validates on the host -- ValueError before any GPU call
(the objects here have no GPU context); and the numpy reference the GPU tests compare against,
pair_reference, the definition of include/fia.h stated row by row over the related list:

    theta_t = (theta_u, theta_i, theta_j),  rel = R_u ++ C_i ++ C_j,  n = |rel|
    H = (2/n) sum_p (g_p g_p^T + e_p d2 r-hat_p) + wd diag(M) + damping I
    v = d (r-hat(u, i) - r-hat(u, j)) / d theta_t,  x = H^-1 v  (one np.linalg.solve)
    influence_p = x . (2 e_p g_p + wd M theta_t) / n,  diff = r-hat(u, i) - r-hat(u, j)

in the extended reference theta order (MF [p_u, q_i, q_j, b_u, b_i, b_j], NCF [Pm_u, Qm_i, Qm_j,
Pg_u, Qg_i, Qg_j]).  It is checked against a torch double-backward over the three slices (built on
oracle/autograd_oracle.py's graphs), against the block assembly from the entity Grams and the
train-pair terms that the kernel performs, and for the swap property.  The problem is that of
tests/test_newton_cpu.py; pair_list builds the batch that tests/test_gpu_pair.py runs, and every
pair of it is asserted here to give cond(H) < 1e8."""
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

SIZES = [("MF", 8), ("MF", 16), ("MF", 32), ("NCF", 8), ("NCF", 16)]


def pair_blocks(model, k):
    """Index arrays of the user, item-i and item-j blocks in the extended reference theta order."""
    idx = np.arange(k)
    if model == "MF":
        return [np.concatenate([b * k + idx, [3 * k + b]]) for b in range(3)]
    return [np.concatenate([b * k + idx, 3 * k + b * k + idx]) for b in range(3)]


def pair_model(model, p, k, u, i, j):
    """(theta_t, M, predict(a, b), gradient(a, b) [D3], C_i, C_j) of the pair (u, i, j): the gradient of
    r-hat(a, b) in theta_t has its user block zero unless a == u, its i block unless b == i, its j
    block unless b == j; C_i / C_j are d2 r-hat / d theta_t^2 of the own pairs (u, i) / (u, j)."""
    idx = np.arange(k)
    if model == "MF":
        P, Q, bu, bi, g = fo._mf_tables(p, k)
        D3 = 3 * k + 3
        theta = np.concatenate([P[u], Q[i], Q[j], [bu[u]], [bi[i]], [bi[j]]])
        M = np.concatenate([np.ones(3 * k), np.zeros(3)])

        def predict(a, b):
            return float(P[a] @ Q[b] + bu[a] + bi[b] + g)

        def gradient(a, b):
            G = np.zeros(D3)
            if a == u:
                G[0:k], G[3 * k] = Q[b], 1.0
            if b == i:
                G[k:2 * k], G[3 * k + 1] = P[a], 1.0
            if b == j:
                G[2 * k:3 * k], G[3 * k + 2] = P[a], 1.0
            return G
        Ci, Cj = np.zeros((D3, D3)), np.zeros((D3, D3))
        Ci[idx, k + idx] = Ci[k + idx, idx] = 1.0
        Cj[idx, 2 * k + idx] = Cj[2 * k + idx, idx] = 1.0
    else:
        T = fo._ncf_tables(p, k)
        D3 = 6 * k
        theta = np.concatenate([T["Pm"][u], T["Qm"][i], T["Qm"][j], T["Pg"][u], T["Qg"][i], T["Qg"][j]])
        M = np.ones(D3)
        W3g = T["W3"][k // 2:]

        def predict(a, b):
            return float(fo.ncf_forward_backward(T, k, [a], [b])[0][0])

        def gradient(a, b):
            _, dPm, dQm, dPg, dQg = fo.ncf_forward_backward(T, k, [a], [b])
            G = np.zeros(D3)
            if a == u:
                G[0:k], G[3 * k:4 * k] = dPm[0], dPg[0]
            if b == i:
                G[k:2 * k], G[4 * k:5 * k] = dQm[0], dQg[0]
            if b == j:
                G[2 * k:3 * k], G[5 * k:6 * k] = dQm[0], dQg[0]
            return G
        Ci, Cj = np.zeros((D3, D3)), np.zeros((D3, D3))
        Ci[3 * k + idx, 4 * k + idx] = Ci[4 * k + idx, 3 * k + idx] = W3g
        Cj[3 * k + idx, 5 * k + idx] = Cj[5 * k + idx, 3 * k + idx] = W3g
    return theta, M, predict, gradient, Ci, Cj


def pair_reference(model, p, k, tu, ti, tr, u, i, j, wd, damping):
    """The definition in numpy, row by row over rel.  Returns dict(rel, n, H, v, x, influence, diff,
    cond, theta, G [n, D3], e [n]); n = 0 gives NaN H / x / cond and no influence."""
    tu, ti = np.asarray(tu), np.asarray(ti)
    y = np.asarray(tr, np.float32).astype(np.float64)
    rel = np.concatenate([np.nonzero(tu == u)[0], np.nonzero(ti == i)[0], np.nonzero(ti == j)[0]]).astype(np.int64)
    n = rel.size
    theta, M, predict, gradient, Ci, Cj = pair_model(model, p, k, u, i, j)
    D3 = theta.size
    v = gradient(u, i) - gradient(u, j)
    diff = predict(u, i) - predict(u, j)
    if n == 0:
        return dict(rel=rel, n=0, H=np.full((D3, D3), np.nan), v=v, x=np.full(D3, np.nan), influence=np.zeros(0),
                    diff=diff, cond=np.nan, theta=theta, G=np.zeros((0, D3)), e=np.zeros(0))
    H = np.zeros((D3, D3))
    G, e = np.zeros((n, D3)), np.zeros(n)
    for pos, row in enumerate(rel):
        a, b = int(tu[row]), int(ti[row])
        e[pos] = predict(a, b) - y[row]
        G[pos] = gradient(a, b)
        H += np.outer(G[pos], G[pos])
        if a == u and b == i:
            H += e[pos] * Ci
        if a == u and b == j:
            H += e[pos] * Cj
    H = (2.0 / n) * H + np.diag(wd * M + damping)
    # one solve, with the item blocks in ascending item order: LAPACK's pivoting depends on the order
    # of the unknowns, and a swapped pair then factorises the same matrix (measured without it: the
    # swap property of x held to 1.05e-14 of max|x| instead of 1e-14)
    blocks = pair_blocks(model, k)
    perm = np.concatenate([blocks[0], blocks[1], blocks[2]] if i < j else [blocks[0], blocks[2], blocks[1]])
    with _one_blas_thread():
        x = np.zeros(D3)
        x[perm] = np.linalg.solve(H[np.ix_(perm, perm)], v[perm])
        cond = float(np.linalg.cond(H))
    infl = (2.0 * e[:, None] * G + (wd * M * theta)[None, :]) @ x / n
    return dict(rel=rel, n=n, H=H, v=v, x=x, influence=infl, diff=diff, cond=cond, theta=theta, G=G, e=e)


def pair_list(tu, ti):
    """The twelve pairs of tests/test_gpu_pair.py (the table of the call's issue): both own pairs with a
    300-entry user list crossing a tile; C_j empty; the duplicated own pair; uncoupled; the empty
    user; item lists of 15 / 16 / 17; both own pairs with short lists; item lists of 1; one own
    pair; the swap of the second pair; and the first pair again."""
    i0 = 7
    free = [b for b in range(40) if not ((tu == DUP[0]) & (ti == b)).any() and (ti == b).sum() >= 4]
    i4, i5 = free[0], free[1]
    assert i4 == queries(tu, ti)[4][1]
    return [(0, i0, 8), (0, i0, 318), (DUP[0], DUP[1], i4), (DUP[0], i4, i5), (19, i0, 300), (18, 300, 301),
            (18, 301, 302), (18, 1, 2), (0, 299, 40), (17, 302, 301), (0, 318, i0), (0, i0, 8)]


def autograd_pair(model, p, k, tu, ti, tr, u, i, j, wd, damping):
    """H, v and the influences of the pair system by torch double backward over the three slices,
    following oracle/autograd_oracle.query: total_loss over the fed related rows, first backprop over
    all parameters sliced to theta_t, second backprop per unit vector, + damping."""
    import torch
    from oracle import autograd_oracle as ao
    build = ao._mf_graph if model == "MF" else ao._ncf_graph
    plist, logits, decayed = build(p, k, U, I)
    if model == "MF":
        sl = [(0, u * k, k), (1, i * k, k), (1, j * k, k), (2, u, 1), (3, i, 1), (3, j, 1)]
    else:
        sl = [(0, u * k, k), (1, i * k, k), (1, j * k, k), (2, u * k, k), (3, i * k, k), (3, j * k, k)]
    D3 = sum(s[2] for s in sl)
    rel = np.concatenate([np.nonzero(tu == u)[0], np.nonzero(ti == i)[0], np.nonzero(ti == j)[0]])
    n = rel.size
    users = torch.tensor(tu[rel], dtype=torch.long)
    items = torch.tensor(ti[rel], dtype=torch.long)
    y = torch.tensor(np.asarray(tr, np.float32).astype(np.float64)[rel])

    def total_loss(us, its, ys):
        return ((logits(us, its) - ys) ** 2).mean() + sum(0.5 * (q ** 2).sum() for q in decayed) * wd

    def sliced(grads):
        grads = [torch.zeros_like(q) if g is None else g for q, g in zip(plist, grads)]
        return torch.cat([grads[pi].reshape(-1)[s:s + L] for pi, s, L in sl])

    d = (logits(torch.tensor([u]), torch.tensor([i])) - logits(torch.tensor([u]), torch.tensor([j]))).squeeze()
    v = sliced(torch.autograd.grad(d, plist, allow_unused=True)).detach().numpy()
    g1s = sliced(torch.autograd.grad(total_loss(users, items, y), plist, create_graph=True))
    H = np.zeros((D3, D3))
    for c in range(D3):
        unit = torch.zeros(D3, dtype=torch.float64)
        unit[c] = 1.0
        H[:, c] = sliced(torch.autograd.grad((g1s * unit).sum(), plist, retain_graph=True,
                                             allow_unused=True)).detach().numpy()
    H += damping * np.eye(D3)
    x = np.linalg.solve(H, v)
    infl = np.zeros(n)
    for r in range(n):
        gr = sliced(torch.autograd.grad(total_loss(users[r:r + 1], items[r:r + 1], y[r:r + 1]), plist,
                                        allow_unused=True)).detach().numpy()
        infl[r] = x @ gr / n
    return dict(H=H, v=v, influence=infl)


@pytest.mark.parametrize("model,k", [("MF", 8), ("NCF", 8)])
def test_reference_against_autograd(model, k):
    """Both own pairs in train, one in train, none: H, v and the influences within 1e-10 of the
    largest entry."""
    tu, ti, tr = problem()
    p = params_for(model, k)
    pairs = pair_list(tu, ti)
    for (u, i, j), owns in ((pairs[0], 2), (pairs[1], 1), (pairs[3], 0)):
        assert int(((tu == u) & (ti == i)).any()) + int(((tu == u) & (ti == j)).any()) == owns
        ref = pair_reference(model, p, k, tu, ti, tr, u, i, j, WD, DAMP)
        ag = autograd_pair(model, p, k, tu, ti, tr, u, i, j, WD, DAMP)
        for key in ("H", "v", "influence"):
            err = np.abs(ref[key] - ag[key]).max() / np.abs(ag[key]).max()
            print("%s k=%d pair %s %s: %.2e" % (model, k, (u, i, j), key, err))
            assert err < 1e-10, ((u, i, j), key, err)


def block_assembly(model, p, k, tu, ti, tr, u, i, j, wd, damping, ref):
    """H from the entity Grams A_u, B_i, B_j and the pair terms (cd, es), as the kernel assembles it."""
    y = np.asarray(tr, np.float32).astype(np.float64)
    theta, M, predict, gradient, Ci, Cj = pair_model(model, p, k, u, i, j)
    bu, bi, bj = pair_blocks(model, k)
    D3, n = theta.size, ref["n"]

    def gram(rows, blk):
        S = np.zeros((blk.size, blk.size))
        for row in rows:
            g = gradient(int(tu[row]), int(ti[row]))[blk]
            S += np.outer(g, g)
        return S
    A_u, B_i, B_j = gram(np.nonzero(tu == u)[0], bu), gram(np.nonzero(ti == i)[0], bi), gram(np.nonzero(ti == j)[0], bj)
    H = np.zeros((D3, D3))
    H[np.ix_(bu, bu)] = A_u
    H[np.ix_(bi, bi)] = B_i
    H[np.ix_(bj, bj)] = B_j
    for item, blk, C in ((i, bi, Ci), (j, bj, Cj)):
        own = np.nonzero((tu == u) & (ti == item))[0]
        cd = own.size
        if not cd:
            continue
        es = cd * predict(u, item) - y[own].sum()
        vv = gradient(u, item)                         # v^i or v^j: user block and the item's block
        H[np.ix_(bu, bu)] += cd * np.outer(vv[bu], vv[bu])
        H[np.ix_(blk, blk)] += cd * np.outer(vv[blk], vv[blk])
        cross = 2.0 * (cd * np.outer(vv[blk], vv[bu]) + es * C[np.ix_(blk, bu)])
        H[np.ix_(blk, bu)] += cross
        H[np.ix_(bu, blk)] += cross.T
    return (2.0 / n) * H + np.diag(wd * M + damping)


@pytest.mark.parametrize("model,k", SIZES)
def test_block_assembly_conditioning_and_swap(model, k):
    """Every pair of the GPU test's batch: the block assembly equals the definition's H to
    1e-12 * max|H|; cond(H) < 1e8, none skipped; swapping i and j negates every influence and the
    gap and swaps and negates the item blocks of x."""
    tu, ti, tr = problem()
    p = params_for(model, k)
    bu, bi, bj = pair_blocks(model, k)
    worst_cond, worst_swap, worst_asm = 0.0, 0.0, 0.0
    for (u, i, j) in pair_list(tu, ti)[:-1]:
        ref = pair_reference(model, p, k, tu, ti, tr, u, i, j, WD, DAMP)
        assert ref["n"] > 0 and np.isfinite(ref["x"]).all()
        Hb = block_assembly(model, p, k, tu, ti, tr, u, i, j, WD, DAMP, ref)
        err = np.abs(Hb - ref["H"]).max() / np.abs(ref["H"]).max()
        worst_asm = max(worst_asm, err)
        assert err < 1e-12, ((u, i, j), err)
        assert ref["cond"] < COND_MAX, ((u, i, j), ref["cond"])
        worst_cond = max(worst_cond, ref["cond"])
        sw = pair_reference(model, p, k, tu, ti, tr, u, j, i, WD, DAMP)
        du, di, dj = (tu == u).sum(), (ti == i).sum(), (ti == j).sum()
        back = np.concatenate([np.arange(du), du + dj + np.arange(di), du + np.arange(dj)])   # rel positions of sw
        assert np.array_equal(sw["rel"][back], ref["rel"]) and sw["diff"] == -ref["diff"]
        scale = np.abs(ref["influence"]).max()
        e_inf = np.abs(sw["influence"][back] + ref["influence"]).max() / scale
        xs = np.zeros_like(ref["x"])
        xs[bu], xs[bi], xs[bj] = -sw["x"][bu], -sw["x"][bj], -sw["x"][bi]
        e_x = np.abs(xs - ref["x"]).max() / np.abs(ref["x"]).max()
        worst_swap = max(worst_swap, e_inf, e_x)
        assert e_inf < 1e-14 and e_x < 1e-14, ((u, i, j), e_inf, e_x)
    print("%s k=%d: largest cond(H) %.3e, block assembly %.2e, swap %.2e" % (model, k, worst_cond, worst_asm,
                                                                              worst_swap))


def test_pair_list_holds_what_the_gpu_test_needs():
    tu, ti, tr = problem()
    pairs = pair_list(tu, ti)
    own = lambda u, b: int(((tu == u) & (ti == b)).sum())
    n = lambda u, i, j: int((tu == u).sum() + (ti == i).sum() + (ti == j).sum())
    assert len(pairs) == 12 and pairs[0] == pairs[-1] == (0, 7, 8) and pairs[10] == (0, 318, 7)
    assert [own(u, i) + own(u, j) for (u, i, j) in pairs] == [2, 1, 2, 0, 0, 0, 0, 2, 2, 1, 1, 2]
    assert own(*DUP) == 2 and pairs[2][:2] == DUP
    assert (tu == 0).sum() == 300 and (ti == 318).sum() == 0 and (tu == 19).sum() == 0
    assert [int((ti == b).sum()) for b in (300, 301, 302, 299, 40)] == [15, 16, 17, 1, 1]
    assert all(n(*q) > 0 and q[1] != q[2] for q in pairs) and n(19, 318, 319) == 0
    assert n(0, 7, 8) > 256                              # the first query's list crosses a scoring tile


# ------------------------------------------------------------------------------------------
# ABI and facade
# ------------------------------------------------------------------------------------------
def test_pair_calls_declared_exported_bound(libfia_path):
    for name in ("fia_count_related_pair", "fia_pair_batch"):
        assert name in header_functions()
        assert hasattr(ctypes.CDLL(libfia_path), name)
        assert name in _lib.SIGNATURES
    lib = _lib.load_library(libfia_path)
    assert lib.fia_count_related_pair(None, 0, None, None, None, None, None, None) == 1
    assert lib.fia_pair_batch(None, 0, None, None, None, None, 0, None, None, None, None, 0, None, None, None,
                              None) == 1
    assert lib.fia_version() == 100


@pytest.mark.parametrize("cls", [MF, NCF])
def test_pair_batch_host_validation(cls):
    m = cls.__new__(cls)          # no GPU context: only the host-side validation is exercised
    m.num_users, m.num_items, m.embedding_size, m.num_train_examples = 7, 5, 8, 20
    m.data_sets = {"test": types.SimpleNamespace(x=np.array([[0, 1], [3, 4]]))}
    for bad in ([2], [2, 3, 4],                          # a length mismatch
                [2.5, 3.0], np.array([2.0, 3.0]),        # not integers
                [-1, 3], [2, 5],                         # out of range
                [[2, 3]],                                # not 1-d
                [1, 3], [2, 4]):                         # j == i_t
        with pytest.raises(ValueError):
            m.get_pair_influence_batch([0, 1], bad, K=1)
    for K in (-1, _lib.FIA_MAX_TOPK + 1, 1.5, True):
        with pytest.raises(ValueError):
            m.get_pair_influence_batch([0, 1], [2, 3], K=K)
    with pytest.raises(ValueError):
        m.prepare_for([0, 1], other_items=[2])
    assert m._checked_other_items([0, 1], [2, 3], distinct=True).tolist() == [2, 3]
    assert m._checked_other_items([0, 1], [1, 4]).dtype == np.int32      # prepare_for's j may be the own item
