"""CPU check of the decomposition the large-k group and self kernels rest on ("Group and
self influence at large k"): for query q = (u, i) and a group S, H - H_S is the base coupled
system of the large-k solver with

    A_u  -> A_u - dA_u,  dA_u = sum_{j in S, on_u} g_ju g_ju^T   (own-pair listings included, once)
    B_i  -> B_i - dB_i   likewise
    cdup -> cdup - c_S   (same-side rank-1 terms and the cross block)
    esum -> esum - e_S   (the cross block's C term)
    wd   -> wd (1 - m_S / n) on the decayed diagonal, the damping unchanged

and b_S, block by block, is (2/n) (sum_{on side} e_j g_j,side + e_S v_side) + (m_S / n) wd M theta.
Built here in numpy from the per-side Grams, the four scalars and v, exactly as the kernels read
them, and compared with group_reference's H - H_S and b_S (tests/test_group_cpu.py), which
restates include/fia.h's definition occurrence by occurrence.

Bound: both sides are sums of the same few hundred products in another order, so they differ by
rounding only: max abs difference <= 1e-12 * max|H| for the matrix, and for the right-hand side
<= 1e-12 * the smaller of max|H| and max|b_S|.  These tests run no kernel: they hold the derivation
the kernels are written from; the tests that fail without the feature are the GPU ones.
"""
import numpy as np
import pytest

from influence import synth
from oracle import fia_oracle as fo
from test_group_cpu import group_reference, w3g_of
from test_gpu_group import DAMP, DUP, I, U, WD, build_groups, problem, queries

K = 8


def blocks(model, k):
    """Reference-order indices of the user block and the item block, and M on each."""
    a = np.arange(k)
    if model == "MF":
        ub, ib = np.concatenate([a, [2 * k]]), np.concatenate([k + a, [2 * k + 1]])
        m = np.concatenate([np.ones(k), [0.0]])
    else:
        ub, ib = np.concatenate([a, 2 * k + a]), np.concatenate([k + a, 3 * k + a])
        m = np.ones(2 * k)
    return ub, ib, m


def decomposed(model, k, core, S, tu, ti, u, i, wd, damping, W3g):
    """(H - H_S, b_S) in the reference theta order, from the quantities the large-k path keeps."""
    rel, n, v, theta, G, e = core["rel"], core["n"], core["v"], core["theta"], core["G"], core["e"]
    D = theta.size
    ub, ib, m = blocks(model, k)
    nu = int((tu == u).sum())                            # rel: the user's list, then the item's
    Gu, Gi = G[:nu][:, ub], G[nu:][:, ib]
    A, B = Gu.T @ Gu, Gi.T @ Gi                          # the cached Grams: every list row once
    own_rows = np.nonzero((tu == u) & (ti == i))[0]
    cdup = float(own_rows.size)
    e_of = {int(r): float(e[p]) for p, r in enumerate(rel)}
    esum = sum(e_of[int(r)] for r in own_rows)
    vu, vi = v[ub], v[ib]
    # the group: members in list order, m_j = 0 skipped
    dA, dB = np.zeros_like(A), np.zeros_like(B)
    bu, bi = np.zeros(ub.size), np.zeros(ib.size)
    c_S = e_S = m_S = 0.0
    pos_u = {int(r): p for p, r in enumerate(rel[:nu])}
    pos_i = {int(r): nu + p for p, r in enumerate(rel[nu:])}
    for j in np.asarray(S, np.int64).reshape(-1):
        j = int(j)
        on_u, on_i = tu[j] == u, ti[j] == i
        if not (on_u or on_i):
            continue
        if on_u:
            g = G[pos_u[j]][ub]
            dA += np.outer(g, g)
            bu += e_of[j] * g
        if on_i:
            g = G[pos_i[j]][ib]
            dB += np.outer(g, g)
            bi += e_of[j] * g
        if on_u and on_i:
            c_S += 1.0
            e_S += e_of[j]
        m_S += float(on_u) + float(on_i)
    s2n = 2.0 / n
    cd, es = cdup - c_S, esum - e_S
    H = np.zeros((D, D))
    H[np.ix_(ub, ub)] = s2n * (A - dA + cd * np.outer(vu, vu)) + np.diag(wd * m * (1.0 - m_S / n) + damping)
    H[np.ix_(ib, ib)] = s2n * (B - dB + cd * np.outer(vi, vi)) + np.diag(wd * m * (1.0 - m_S / n) + damping)
    cross = s2n * 2.0 * cd * np.outer(vi, vu)            # item rows, user columns
    C = np.zeros((ib.size, ub.size))
    idx = np.arange(k)
    if model == "MF":
        C[idx, idx] = 1.0
    else:
        C[k + idx, k + idx] = W3g
    cross += s2n * 2.0 * es * C
    H[np.ix_(ib, ub)] = cross
    H[np.ix_(ub, ib)] = cross.T
    b = np.zeros(D)
    b[ub] = s2n * (bu + e_S * vu) + (m_S / n) * wd * m * theta[ub]
    b[ib] = s2n * (bi + e_S * vi) + (m_S / n) * wd * m * theta[ib]
    return H, b


@pytest.mark.parametrize("model", ["MF", "NCF"])
def test_decomposition_matches_group_reference(model):
    tu, ti, tr = problem()
    p = synth.mf_params(U, I, K, 3) if model == "MF" else synth.ncf_params(U, I, K, 3)
    W3g = w3g_of(model, p, K)
    qs = queries(tu, ti)
    named = build_groups(tu, ti, qs)
    dup_rows = np.nonzero((tu == DUP[0]) & (ti == DUP[1]))[0]
    own0 = np.nonzero((tu == qs[0][0]) & (ti == qs[0][1]))[0]
    g0 = dict(named[0])
    cases = [(0, "user", g0["user"]), (0, "item", g0["item"]), (0, "mixed", g0["mixed"]),
             (0, "own alone", own0), (0, "own", g0["own"]), (0, "wide", g0["wide"]),
             (0, "user+unrelated", g0["user+unrelated"]),
             (1, "dup-one", dup_rows[:1]), (1, "dup-both", dup_rows), (1, "dup-both+", dict(named[1])["dup-both+"]),
             (4, "with-dup", dict(named[4])["with-dup"]),     # the pair's rows as user-side members, m = 1
             (2, "user-only-query", dict(named[2])["user-only-query"]),
             (3, "item-only-query", dict(named[3])["item-only-query"])]
    cores = {}
    for q, name, rows in cases:
        u, i = qs[q]
        if q not in cores:
            cores[q] = fo.query(model, p, K, tu, ti, tr, u, i, WD, DAMP)
        core = cores[q]
        ref = group_reference(core, rows, WD, DAMP, W3g)
        want_H = core["H"] - ref["H_S"]
        H, b = decomposed(model, K, core, rows, tu, ti, u, i, WD, DAMP, W3g)
        dh = np.abs(H - want_H).max()
        db = np.abs(b - ref["b_S"]).max()
        print("%s q%d %-16s |dH| %.2e (max|H| %.2e)  |db| %.2e (max|b| %.2e)" % (
            model, q, name, dh, np.abs(core["H"]).max(), db, np.abs(ref["b_S"]).max()))
        assert dh <= 1e-12 * np.abs(core["H"]).max(), (q, name)
        assert db <= 1e-12 * min(np.abs(ref["b_S"]).max(), np.abs(core["H"]).max()), (q, name)
        # and so the solve: the decomposed system gives the reference's dtheta
        dth = np.linalg.solve(H, b)
        assert np.abs(dth - ref["dtheta"]).max() <= 1e-9 * np.abs(ref["dtheta"]).max(), (q, name)
