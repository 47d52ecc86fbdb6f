"""CPU tests of the per-rating Newton call: fia_query_batch_newton is declared, exported and bound
and refuses a NULL context; the facade validates on the host -- ValueError before any GPU call (the
objects here have no GPU context); and the numpy reference the GPU tests compare against,
newton_reference, whose two routes must agree:

  * the definition: per related position p, group_reference(core, [rel[p]], ...)["group"]
    (tests/test_group_cpu.py), i.e. v . (H - H_{j})^-1 b_{j} with one solve per position;
  * the closed form of include/fia.h for m_j = 1 positions (every row but the own pair):
        H' = H - (wd/n) diag(M), c = 2/n, x' = H'^-1 v, w' = H'^-1 (wd M theta)/n, c' = x' . (wd M theta)/n
        s = x' . g, t = w' . g, h = g^T H'^-1 g
        newton = 2 e s / n + c' + c s (2 e h / n + t) / (1 - c h)

The problem (shared with tests/test_gpu_newton.py): 20 users x 320 items.  User 0 rates items
0 .. 299 (300 = 256 + 44: more than one 256-rating chunk, a tile tail of 12, more than 64); users
1 .. 11 rate 32 of items 0 .. 39 (item lists of about 10); items 300 / 301 / 302 are rated by
users 1 .. 15 / 16 / 17 (item lists of 15, 16 and 17: one short of, exactly and one past a
16-rating tile -- which takes more than the 14 users the first sketch of this problem had);
items 40 .. 299 have user 0's rating alone (lists of 1); (3, 5) is present twice with different
ratings; user 18 has three ratings; user 19 and items 318 and 319 have none; rows are shuffled."""
import ctypes

import numpy as np
import pytest

from influence import _lib, synth
from influence.NCF import NCF
from influence.matrix_factorization import MF
from oracle import fia_oracle as fo

from test_abi import header_functions
from test_group_cpu import group_reference, w3g_of

WD, DAMP = 1e-3, 1e-6
U, I = 20, 320
HEAVY = 300
DUP = (3, 5)


def problem():
    rng = np.random.default_rng(33)
    rows = [(0, b) for b in range(HEAVY)]
    for a in range(1, 12):
        items = [int(b) for b in rng.choice(40, 32, replace=False)]
        if a == DUP[0]:
            items = [b for b in items if b != DUP[1]][:31] + [DUP[1], DUP[1]]
        rows += [(a, b) for b in items]
    for item, last in ((300, 15), (301, 16), (302, 17)):
        rows += [(a, item) for a in range(1, last + 1)]
    rows += [(18, 1), (18, 2), (18, 310)]
    tu = np.array([r[0] for r in rows], np.int32)
    ti = np.array([r[1] for r in rows], np.int32)
    tr = (rng.random(len(rows)) * 4.0 + 1.0).astype(np.float32)
    perm = rng.permutation(len(rows))                   # a train row is not its list position
    tu, ti, tr = tu[perm], ti[perm], tr[perm]
    d = np.nonzero((tu == DUP[0]) & (ti == DUP[1]))[0]
    assert d.size == 2 and tr[d[0]] != tr[d[1]]
    assert (tu == 0).sum() == HEAVY and (tu == 19).sum() == 0 and (ti >= 318).sum() == 0
    assert [(ti == b).sum() for b in (299, 300, 301, 302)] == [1, 15, 16, 17]
    return tu, ti, tr


def queries(tu, ti):
    """A train row of user 0; the duplicated pair; user 0 with an unrated item (user side only);
    the empty user with a rated item (item side only); a non-train pair; n_q = 0; item lists of
    15, 16 (two consecutive queries on that item), 17 and 1; and the first pair again."""
    i0 = 7
    assert ((tu == 0) & (ti == i0)).sum() == 1 and (ti == i0).sum() >= 6
    i4 = next(b for b in range(40) if not ((tu == DUP[0]) & (ti == b)).any() and (ti == b).sum() >= 4)
    return [(0, i0), DUP, (0, 318), (19, i0), (DUP[0], i4), (19, 319), (18, 300), (18, 301), (19, 301), (18, 302),
            (18, 299), (0, i0)]


def _one_blas_thread():
    """Hundreds of solves of systems of at most 130 unknowns: a threaded BLAS spends its time
    handing them out (MF k=64: 46 s against 2 s).  Without threadpoolctl nothing is limited."""
    try:
        from threadpoolctl import threadpool_limits
        return threadpool_limits(limits=1)
    except ImportError:
        import contextlib
        return contextlib.nullcontext()


def newton_reference(core, wd, damping, W3g=None):
    """Per related position of an oracle query: dict(newton [n] by the definition, closed [n] by
    the closed form (NaN at own-pair positions), own [n] bool, cond [n] of H - H_j, min_den the
    smallest |1 - c h| met)."""
    rel, n, v, H, theta, G, e = core["rel"], core["n"], core["v"], core["H"], core["theta"], core["G"], core["e"]
    D = theta.size
    ncf = W3g is not None
    k = D // 4 if ncf else (D - 2) // 2
    M = np.ones(D) if ncf else np.concatenate([np.ones(2 * k), np.zeros(2)])
    own = np.array([np.count_nonzero(rel == r) == 2 for r in rel], bool)
    newton, cond = np.zeros(n), np.zeros(n)
    with _one_blas_thread():
        for p in range(n):
            ref = group_reference(core, [rel[p]], wd, damping, W3g)
            newton[p], cond[p] = ref["group"], ref["cond"]
    Hp = H - np.diag(wd * M) / n
    rhs = wd * M * theta / n
    xp, wp = np.linalg.solve(Hp, v), np.linalg.solve(Hp, rhs)
    cp, c = float(xp @ rhs), 2.0 / n
    PG = np.linalg.solve(Hp, G.T).T                     # rows: H'^-1 g_p
    s, t, h = G @ xp, G @ wp, np.einsum("pd,pd->p", G, PG)
    den = 1.0 - c * h
    closed = 2.0 * e * s / n + cp + c * s * (2.0 * e * h / n + t) / den
    closed[own] = np.nan
    return dict(newton=newton, closed=closed, own=own, cond=cond,
                min_den=float(np.abs(den[~own]).min()) if (~own).any() else np.inf)


@pytest.mark.parametrize("model,k", [("MF", 8), ("NCF", 8)])
def test_closed_form_is_the_singleton_group(model, k):
    tu, ti, tr = problem()
    p = synth.mf_params(U, I, k, 3) if model == "MF" else synth.ncf_params(U, I, k, 3)
    W3g = w3g_of(model, p, k)
    min_den, seen_own = np.inf, 0
    for (u, i) in queries(tu, ti)[:-1]:
        core = fo.query(model, p, k, tu, ti, tr, u, i, WD, DAMP)
        if not core["n"]:
            continue
        ref = newton_reference(core, WD, DAMP, W3g)
        live = ~ref["own"]
        seen_own += int(ref["own"].sum())
        scale = np.abs(ref["newton"]).max()
        err = np.abs(ref["closed"][live] - ref["newton"][live]).max() / scale
        min_den = min(min_den, ref["min_den"])
        assert err < 1e-9, ((u, i), err)
        # both positions of an own-pair row hold the same value
        for r in np.unique(core["rel"][ref["own"]]):
            a, b = np.nonzero(core["rel"] == r)[0]
            assert ref["newton"][a] == ref["newton"][b]
    assert seen_own == 2 + 4                            # (0, i0): one row; the duplicated pair: two rows
    print("smallest |1 - c h| %.3e" % min_den)


def test_query_batch_newton_declared_exported_bound(libfia_path):
    assert "fia_query_batch_newton" in header_functions()
    assert hasattr(ctypes.CDLL(libfia_path), "fia_query_batch_newton")
    assert "fia_query_batch_newton" in _lib.SIGNATURES
    lib = _lib.load_library(libfia_path)
    assert lib.fia_query_batch_newton(None, 0, None, None, None, 0, None, None, 0, None, None, None, None) == 1
    assert lib.fia_version() == 100


@pytest.mark.parametrize("cls", [MF, NCF])
def test_newton_batch_host_validation(cls):
    m = cls.__new__(cls)          # no GPU context: only the host-side validation is exercised
    m.num_users, m.num_items, m.embedding_size, m.num_train_examples = 7, 5, 8, 20
    for kwargs in (dict(K=-1), dict(K=_lib.FIA_MAX_TOPK + 1), dict(K=1.5), dict(K=True), dict(K=0, full=False)):
        with pytest.raises(ValueError):
            m.get_newton_influence_batch([0, 1], **kwargs)
    for bad in ([[0, 1]], [0.5], [-1, 0], np.array([1.0, 2.0])):
        with pytest.raises(ValueError):
            m.get_newton_influence_batch(bad, K=1)
