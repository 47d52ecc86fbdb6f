"""CPU tests of the group-removal call: fia_group_influence is declared, exported and bound and
refuses a NULL context; the facade validates the groups on the host -- ValueError before any GPU
call (the objects here have no GPU context); and the pure-numpy reference the GPU tests compare
against, group_reference, checked against the oracle's own H and influences.

group_reference restates include/fia.h's definition from what oracle.fia_oracle._mf_core /
_ncf_core return (rel, n, v, H, x, G, e, theta): the occurrences of S are the positions p of
the related list with rel[p] in S (the test pair's own train row sits there twice), and

    H_S = (1/n) sum_occ (2 G_p G_p^T + 2 e_p C [p is the own pair] + wd M)
    b_S = (1/n) sum_occ (2 e_p G_p + wd M theta)
    dtheta = (H - H_S)^-1 b_S,  group = v . dtheta,  first_order = x . b_S
"""
import ctypes

import numpy as np
import pytest

from influence import _lib, synth
from influence.NCF import NCF
from influence.matrix_factorization import MF
from oracle import fia_oracle as fo

from test_abi import header_functions


def group_reference(core, S, wd, damping, W3g=None):
    """The definition in numpy.  core: an oracle query; S: train rows (a row listed twice counts
    twice); W3g: NCF's h3 weights of the GMF half (the coupling block), None for MF.  Returns
    dict(group, first_order, dtheta, H_S, b_S, occ, cond) -- cond of the downdated system."""
    rel, n, v, H, theta = core["rel"], core["n"], core["v"], core["H"], core["theta"]
    G, e = core["G"], core["e"]
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
    S = np.asarray(S, np.int64).reshape(-1)
    times = np.array([np.count_nonzero(S == r) for r in rel], np.int64)     # listings of each position's row
    own = np.array([np.count_nonzero(rel == r) == 2 for r in rel], bool)    # the own pair is in rel twice
    occ = np.nonzero(times)[0]
    H_S = np.zeros((D, D))
    b_S = np.zeros(D)
    for p in occ:
        t = float(times[p])
        H_S += t / n * (2.0 * np.outer(G[p], G[p]) + (2.0 * e[p] * C if own[p] else 0.0) + np.diag(wd * M))
        b_S += t / n * (2.0 * e[p] * G[p] + wd * M * theta)
    Hd = H - H_S
    dtheta = np.linalg.solve(Hd, b_S) if occ.size else np.zeros(D)
    return dict(group=float(v @ dtheta), first_order=float(core["x"] @ b_S), dtheta=dtheta, H_S=H_S, b_S=b_S,
                occ=occ, cond=float(np.linalg.cond(Hd)))


def w3g_of(model, p, k):
    return None if model == "MF" else np.asarray(p["h3/weights"], np.float64).reshape(-1)[k // 2:]


# ------------------------------------------------------------------------------------------
# the reference against the oracle
# ------------------------------------------------------------------------------------------
WD, DAMP = 1e-3, 1e-6


def _problem(model, k):
    rng = np.random.default_rng(4)
    U, I, N = 9, 14, 70
    key = np.sort(rng.choice(U * I, N, replace=False))
    tu, ti = (key // I).astype(np.int32), (key % I).astype(np.int32)
    tr = rng.integers(1, 6, N).astype(np.float32)
    p = synth.mf_params(U, I, k, 1) if model == "MF" else synth.ncf_params(U, I, k, 1)
    return p, tu, ti, tr


@pytest.mark.parametrize("model,k", [("MF", 8), ("NCF", 8)])
def test_reference_against_oracle(model, k):
    p, tu, ti, tr = _problem(model, k)
    W3g = w3g_of(model, p, k)
    u, i = int(tu[11]), int(ti[11])                     # a train row: its two occurrences are coupled
    core = fo.query(model, p, k, tu, ti, tr, u, i, WD, DAMP)
    n, D = core["n"], core["theta"].size
    assert np.count_nonzero(core["rel"] == 11) == 2
    # a group of one: first_order is the sum of the row's influences (one per occurrence)
    for row in (int(core["rel"][0]), 11, int(core["rel"][-1])):
        ref = group_reference(core, [row], WD, DAMP, W3g)
        assert ref["occ"].size == (2 if row == 11 else 1)
        want = core["influence"][ref["occ"]].sum()
        assert abs(ref["first_order"] - want) <= 1e-12 * max(abs(want), 1e-300)
    # every occurrence removed: what is left of H is the damping
    ref = group_reference(core, np.unique(core["rel"]), WD, DAMP, W3g)
    assert ref["occ"].size == n
    assert np.abs(ref["H_S"] - (core["H"] - DAMP * np.eye(D))).max() <= 1e-12
    # an unrelated row contributes nothing; an empty group is zero
    out = next(j for j in range(len(tr)) if tu[j] != u and ti[j] != i)
    a = group_reference(core, [int(core["rel"][0])], WD, DAMP, W3g)
    b = group_reference(core, [int(core["rel"][0]), out], WD, DAMP, W3g)
    assert a["group"] == b["group"] and np.array_equal(a["dtheta"], b["dtheta"])
    z = group_reference(core, [], WD, DAMP, W3g)
    assert z["group"] == 0.0 and z["first_order"] == 0.0 and not z["dtheta"].any()
    # with the curvature kept the Newton step is the first-order sum
    S = core["rel"][:5]
    ref = group_reference(core, S, WD, DAMP, W3g)
    assert abs(core["v"] @ np.linalg.solve(core["H"], ref["b_S"]) - ref["first_order"]) <= 1e-9 * abs(ref["first_order"])
    assert ref["group"] != ref["first_order"]


# ------------------------------------------------------------------------------------------
# ABI and facade
# ------------------------------------------------------------------------------------------
def test_group_influence_declared_exported_bound(libfia_path):
    assert "fia_group_influence" in header_functions()
    assert hasattr(ctypes.CDLL(libfia_path), "fia_group_influence")
    assert "fia_group_influence" in _lib.SIGNATURES
    lib = _lib.load_library(libfia_path)
    assert lib.fia_group_influence(None, 0, None, None, None, 0, None, 0, None, None, None, None, None) == 1
    assert lib.fia_version() == 100


def _bare(cls, k=8, U=7, I=5, n_train=20):
    m = cls.__new__(cls)          # no GPU context: only the host-side validation is exercised
    m.num_users, m.num_items, m.embedding_size, m.num_train_examples = U, I, k, n_train
    return m


@pytest.mark.parametrize("cls", [MF, NCF])
def test_group_influence_host_validation(cls):
    m = _bare(cls)
    ok = [np.array([1, 2]), np.array([], np.int64)]
    for groups in ([[ok[0]]],                                        # one query's groups for two queries
                   [[ok[0]], [ok[1]], []],                           # three for two
                   [[np.array([1.0, 2.0])], []],                     # not integers
                   [[[0.5]], []],
                   [[np.array([0, 20])], []],                        # past the last train row
                   [[np.array([-1, 3])], []],
                   [[], [ok[0], np.array([4, 7, 4])]],               # a row twice in one group
                   [[np.array([[1, 2]])], []]):                      # not 1-d
        with pytest.raises(ValueError):
            m.get_group_influence([0, 1], groups)
    d = 2 * 8 + 2 if cls is MF else 4 * 8
    with pytest.raises(ValueError):
        m.get_group_influence([0, 1], [[ok[0]], []], inverse_hvp=np.zeros((2, d + 1)))
    # what passes the checks: offsets of the flattened batch (empty groups and queries included)
    go, mo, rows = m._checked_groups(3, [[ok[0], ok[1]], [], [np.array([19]), [3, 4, 5]]])
    assert go.tolist() == [0, 2, 2, 4] and mo.tolist() == [0, 2, 2, 3, 6]
    assert rows.dtype == np.int32 and rows.tolist() == [1, 2, 19, 3, 4, 5]
