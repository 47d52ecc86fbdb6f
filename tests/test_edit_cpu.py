"""CPU tests of the edit-set call: fia_edit_influence is declared, exported and bound and refuses a
NULL context; the facade validates the edit sets on the host -- ValueError before any GPU call (the
objects here have no GPU context); and the numpy reference the GPU tests compare against,
edit_reference, the definition of include/fia.h with one np.linalg.solve per group:

    H_R, b_R    as group_reference (tests/test_group_cpu.py) builds H_S, b_S for the removed rows
    H_A = (1/n) sum_{c in A} (2 g_c g_c^T + 2 e_c C [both] + wd diag(M)),  b_A = (1/n) sum_{c in A} (2 e_c g_c + wd M theta)
    dtheta = (H - H_R + H_A)^-1 (b_R - b_A),  edit = v . dtheta,  first_order = x . (b_R - b_A)

checked at the seven sizes against group_reference (A empty), against the per-candidate definition
of tests/test_cand_newton_cpu.py (R empty, one addition, the sign flipped) and against first order
(H_R and H_A dropped).  The problem and the queries are those of tests/test_newton_cpu.py;
edit_groups builds the groups that tests/test_gpu_edit.py runs, and every one of them is asserted
here to give cond(H - H_R + H_A) < 1e8."""
import ctypes

import numpy as np
import pytest

from influence import _lib
from influence.NCF import NCF
from influence.matrix_factorization import MF
from oracle import fia_oracle as fo

from test_abi import header_functions
from test_cand_newton_cpu import COND_MAX, SIZES, cand_newton_reference, candidate_gradients, params_for
from test_group_cpu import group_reference, w3g_of
from test_newton_cpu import DAMP, DUP, I, U, WD, _one_blas_thread, problem, queries

NO_ADDS = np.zeros((0, 3))


def edit_reference(core, removes, adds, wd, damping, W3g=None):
    """The definition in numpy.  core: an oracle query with n > 0; removes: train rows (a row listed
    twice counts twice, an unrelated row not at all); adds: None or (G [m, D], e [m], both [m]) as
    candidate_gradients returns them; W3g: NCF's h3 weights of the GMF half, None for MF.  Returns
    dict(edit, first_order, dtheta, b, cond) -- cond of the edited system H - H_R + H_A."""
    n, v, H, theta = core["n"], core["v"], core["H"], core["theta"]
    D = theta.size
    ncf = W3g is not None
    k = D // 4 if ncf else (D - 2) // 2
    M = np.ones(D) if ncf else np.concatenate([np.ones(2 * k), np.zeros(2)])
    C = np.zeros((D, D))
    idx = np.arange(k)
    if ncf:
        C[2 * k + idx, 3 * k + idx] = C[3 * k + idx, 2 * k + idx] = W3g
    else:
        C[idx, k + idx] = C[k + idx, idx] = 1.0
    rem = group_reference(core, removes, wd, damping, W3g)
    H_A, b_A = np.zeros((D, D)), np.zeros(D)
    m = 0
    if adds is not None:
        G, e, both = adds
        m = e.size
        for j in range(m):
            H_A += (2.0 * np.outer(G[j], G[j]) + (2.0 * e[j] * C if both[j] else 0.0) + np.diag(wd * M)) / n
            b_A += (2.0 * e[j] * G[j] + wd * M * theta) / n
    He = H - rem["H_S"] + H_A
    b = rem["b_S"] - b_A
    with _one_blas_thread():
        dtheta = np.linalg.solve(He, b) if rem["occ"].size or m else np.zeros(D)
        cond = float(np.linalg.cond(He))
    return dict(edit=float(v @ dtheta), first_order=float(core["x"] @ b), dtheta=dtheta, b=b, cond=cond)


def related_rows(tu, ti, u, i):
    """(related train rows in row order, unrelated train rows in row order) of query (u, i)."""
    on = (tu == u) | (ti == i)
    return np.nonzero(on)[0], np.nonzero(~on)[0]


def mixed_additions(rng, u, i, m):
    """m additions cycling user side, item side, neither (ids never the query's own pair)."""
    out = []
    users = [a for a in range(U) if a != u]
    items = [b for b in range(I) if b != i]
    for j in range(m):
        a, b = int(rng.choice(users)), int(rng.choice(items))
        side = j % 3
        pair = (u, b) if side == 0 else ((a, i) if side == 1 else (a, b))
        out.append((pair[0], pair[1], float(np.float32(rng.random() * 4.0 + 1.0))))
    return np.array(out, np.float64).reshape(-1, 3)


def padded_removals(rel, unrel, m):
    """m distinct train rows: related ones -- never all of them -- then unrelated ones (m_j = 0)."""
    take = rel[:min(m, max(rel.size - 1, 1))]
    return np.concatenate([take, unrel[:m - take.size]]).astype(np.int64)


def edit_groups(tu, ti, tr, u, i, seed):
    """The groups of live query (u, i) in tests/test_gpu_edit.py, as (name, remove_rows int64,
    add_triples float64 [m, 3]): empty; removal-only of 1 and 17 members; addition-only of 1, 2, 16
    and 17 members mixing user side, item side and neither; a mixed group of 20 + 20; one related
    rating replaced by another y; and a `both` addition -- on a train-row query as the replacement
    of its own row, else alone.  Ratings are non-integer, so nothing passes by e = 0."""
    rng = np.random.default_rng(seed)
    rel, unrel = related_rows(tu, ti, u, i)
    own = np.nonzero((tu == u) & (ti == i))[0]
    y = lambda: float(np.float32(rng.random() * 4.0 + 1.0))
    groups = [("empty", np.zeros(0, np.int64), NO_ADDS),
              ("rem1", rel[:1].astype(np.int64), NO_ADDS),
              ("rem17", padded_removals(rel, unrel, 17), NO_ADDS)]
    for m in (1, 2, 16, 17):
        groups.append(("add%d" % m, np.zeros(0, np.int64), mixed_additions(rng, u, i, m)))
    groups.append(("mixed", padded_removals(rel[::-1], unrel[::-1], 20), mixed_additions(rng, u, i, 20)))
    j = int(next(r for r in rel if r not in own))       # an ordinary related row
    groups.append(("replace", np.array([j], np.int64), np.array([[tu[j], ti[j], y()]], np.float64)))
    if own.size:
        groups.append(("replace_own", own[:1].astype(np.int64), np.array([[u, i, y()]], np.float64)))
    else:
        groups.append(("add_both", np.zeros(0, np.int64), np.array([[u, i, y()]], np.float64)))
    return groups


def reference_of(model, p, k, core, u, i, rem, add, W3g):
    adds = candidate_gradients(model, p, k, u, i, add[:, 0], add[:, 1], add[:, 2]) if add.shape[0] else None
    return edit_reference(core, rem, adds, WD, DAMP, W3g)


def live_queries(tu, ti):
    """The distinct queries of the problem with n_q > 0, in order."""
    seen, out = set(), []
    for (u, i) in queries(tu, ti):
        if (u, i) not in seen and ((tu == u).sum() + (ti == i).sum()) > 0:
            seen.add((u, i))
            out.append((u, i))
    return out


@pytest.mark.parametrize("model,k", SIZES)
def test_reference_against_the_existing_references(model, k):
    tu, ti, tr = problem()
    p = params_for(model, k)
    W3g = w3g_of(model, p, k)
    rng = np.random.default_rng(500 + k)
    for (u, i) in live_queries(tu, ti)[:5]:
        core = fo.query(model, p, k, tu, ti, tr, u, i, WD, DAMP)
        rel, unrel = related_rows(tu, ti, u, i)
        # A empty: the group call's definition, unrelated rows and all
        S = np.concatenate([rel[:3], unrel[:2]])
        a, b = edit_reference(core, S, None, WD, DAMP, W3g), group_reference(core, S, WD, DAMP, W3g)
        # (the same matrices; only the BLAS threading of the two solves may differ)
        assert abs(a["edit"] - b["group"]) <= 1e-9 * abs(b["group"]) and a["first_order"] == b["first_order"]
        assert np.abs(a["dtheta"] - b["dtheta"]).max() <= 1e-9 * np.abs(b["dtheta"]).max()
        assert abs(a["cond"] - b["cond"]) <= 1e-6 * b["cond"]
        # R empty, one addition: minus the per-candidate definition, for every kind of candidate
        cu, ci = np.array([u, 5, u, 6]), np.array([11, i, i, 12])
        cu[1] = 5 if u != 5 else 4
        cu[3] = 6 if u != 6 else 4
        ci[0] = 11 if i != 11 else 13
        ci[3] = 12 if i != 12 else 13
        cy = rng.random(4) * 4.0 + 1.0
        G, e, both = candidate_gradients(model, p, k, u, i, cu, ci, cy)
        assert both.tolist() == [False, False, True, False] and not G[3].any()
        cand = cand_newton_reference(core, G, e, both, WD, W3g)
        scale = np.abs(cand["newton"]).max()
        for j in range(4):
            one = edit_reference(core, [], (G[j:j + 1], e[j:j + 1], both[j:j + 1]), WD, DAMP, W3g)
            assert abs(one["edit"] + cand["newton"][j]) <= 1e-9 * scale, ((u, i), j)
            assert abs(one["first_order"] + cand["first"][j]) <= 1e-9 * scale
        # H_R and H_A dropped: first order; kept: something else
        mix = edit_reference(core, rel[:4], (G, e, both), WD, DAMP, W3g)
        first = core["v"] @ np.linalg.solve(core["H"], mix["b"])
        assert abs(first - mix["first_order"]) <= 1e-9 * abs(mix["first_order"])
        assert mix["edit"] != mix["first_order"]
        # nothing edited: zero
        z = edit_reference(core, unrel[:3], None, WD, DAMP, W3g)
        assert z["edit"] == 0.0 and z["first_order"] == 0.0 and not z["dtheta"].any()


@pytest.mark.parametrize("model,k", SIZES)
def test_gpu_test_groups_are_well_conditioned(model, k):
    """Every group tests/test_gpu_edit.py compares against the reference: cond < 1e8, none skipped."""
    tu, ti, tr = problem()
    p = params_for(model, k)
    W3g = w3g_of(model, p, k)
    worst, names = 0.0, set()
    for n_q, (u, i) in enumerate(live_queries(tu, ti)):
        core = fo.query(model, p, k, tu, ti, tr, u, i, WD, DAMP)
        for name, rem, add in edit_groups(tu, ti, tr, u, i, 90 + n_q):
            ref = reference_of(model, p, k, core, u, i, rem, add, W3g)
            assert ref["cond"] < COND_MAX, ((u, i), name, ref["cond"])
            assert np.isfinite(ref["edit"]) and np.isfinite(ref["dtheta"]).all()
            worst = max(worst, ref["cond"])
            names.add(name)
    assert names == {"empty", "rem1", "rem17", "add1", "add2", "add16", "add17", "mixed", "replace", "replace_own",
                     "add_both"}
    print("%s k=%d: largest cond(H - H_R + H_A) %.3e" % (model, k, worst))


def test_edit_groups_hold_what_the_gpu_test_needs():
    tu, ti, tr = problem()
    lq = live_queries(tu, ti)
    assert lq[0] == (0, 7) and lq[1] == DUP and len(lq) == 10
    for n_q, (u, i) in enumerate(lq):
        groups = dict((g[0], g[1:]) for g in edit_groups(tu, ti, tr, u, i, 90 + n_q))
        rel, _ = related_rows(tu, ti, u, i)
        assert groups["rem17"][0].size == 17 and np.unique(groups["rem17"][0]).size == 17
        assert groups["mixed"][0].size == 20 and groups["mixed"][1].shape == (20, 3)
        a = groups["add17"][1]
        on_u, on_i = a[:, 0] == u, a[:, 1] == i
        assert (on_u & ~on_i).sum() == 6 and (~on_u & on_i).sum() == 6 and (~on_u & ~on_i).sum() == 5
        r, a = groups["replace"]
        assert (tu[r[0]], ti[r[0]]) == (a[0, 0], a[0, 1]) and a[0, 2] != tr[r[0]] and r[0] in rel
        if "replace_own" in groups:
            r, a = groups["replace_own"]
            assert (tu[r[0]], ti[r[0]]) == (u, i) == (a[0, 0], a[0, 1])
        else:
            assert not ((tu == u) & (ti == i)).any() and tuple(groups["add_both"][1][0, :2]) == (u, i)


# ------------------------------------------------------------------------------------------
# ABI and facade
# ------------------------------------------------------------------------------------------
def test_edit_influence_declared_exported_bound(libfia_path):
    assert "fia_edit_influence" in header_functions()
    assert hasattr(ctypes.CDLL(libfia_path), "fia_edit_influence")
    assert "fia_edit_influence" in _lib.SIGNATURES
    lib = _lib.load_library(libfia_path)
    rc = lib.fia_edit_influence(None, 0, None, None, None, 0, None, 0, None, None, 0, None, None, None, None, None,
                                None, 0, None, None, None)
    assert rc == 1
    assert lib.fia_version() == 100


@pytest.mark.parametrize("cls", [MF, NCF])
def test_edit_influence_host_validation(cls):
    m = cls.__new__(cls)          # no GPU context: only the host-side validation is exercised
    m.num_users, m.num_items, m.embedding_size, m.num_train_examples = 7, 5, 8, 20
    rows, adds = np.array([1, 2]), [(0, 1, 3.5), (6, 4, 1.5)]
    ok = (rows, adds)
    for edits in ([[ok]],                                            # one query's groups for two queries
                  [[ok], [], []],                                    # three for two
                  [[rows], []],                                      # not a pair
                  [[(rows, adds, adds)], []],
                  [[(np.array([1.0, 2.0]), adds)], []],              # rows not integers
                  [[(np.array([0, 20]), adds)], []],                 # past the last train row
                  [[(np.array([-1, 3]), adds)], []],
                  [[(np.array([4, 7, 4]), adds)], []],               # a row twice in one group
                  [[(np.array([[1, 2]]), adds)], []],                # not 1-d
                  [[(rows, [(0, 1)])], []],                          # not triples
                  [[(rows, [(0, 1, 2.0), (1, 2)])], []],             # ragged
                  [[(rows, [(0.5, 1, 2.0)])], []],                   # not an integer id
                  [[(rows, [(7, 1, 2.0)])], []],                     # user id out of range
                  [[(rows, [(0, -1, 2.0)])], []],                    # item id out of range
                  [[(rows, [(0, 1, np.nan)])], []],                  # not a rating
                  [[(rows, [("a", 1, 2.0)])], []]):
        with pytest.raises(ValueError):
            m.get_edit_influence([0, 1], edits)
    for K in (-1, _lib.FIA_MAX_TOPK + 1, 1.5, True):
        with pytest.raises(ValueError):
            m.get_edit_influence([0, 1], [[ok], []], K=K)
    # what passes the checks: offsets of the flattened batch (empty lists, groups and queries included)
    go, ro, rr, ao, au, ai, ay = m._checked_edits(3, [[ok, ([], [])], [], [(np.array([19]), []), ([], adds[:1])]])
    assert go.tolist() == [0, 2, 2, 4] and ro.tolist() == [0, 2, 2, 3, 3] and ao.tolist() == [0, 2, 2, 2, 3]
    assert rr.dtype == np.int32 and rr.tolist() == [1, 2, 19]
    assert au.dtype == np.int32 and au.tolist() == [0, 6, 0] and ai.tolist() == [1, 4, 1]
    assert ay.dtype == np.float32 and ay.tolist() == [3.5, 1.5, 3.5]
