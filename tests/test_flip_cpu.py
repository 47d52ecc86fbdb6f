"""CPU tests of the flip call: fia_pair_flip is declared, exported and bound and refuses a NULL
context; the facade validates on the host -- ValueError before any GPU call (the objects here have
no GPU context); and the numpy reference the GPU tests compare against, flip_reference, the
definition of include/fia.h built on pair_reference (tests/test_pair_cpu.py):

    val_p = the pair influence at position p of R_u;  eligible: item not in {i, j} and val_p < 0
    S = eligible positions by (val, position) -- one stable sort -- taken while fewer than max_set are
        taken, one is left and (diff + margin) + running sum >= 0
    H_S = (1/n) sum_S (2 g g^T + wd diag(M)),  b_S = (1/n) sum_S (2 e g + wd M theta_t)
    dtheta = (H - H_S)^-1 b_S  (one np.linalg.solve),  newton = v . dtheta,  first_order = sum_S val

The downdate is checked independently (H - H_S against the H rebuilt row by row over rel without
S, x . b_S against the summed values).  flip_cases names the cases tests/test_gpu_flip.py runs --
pairs of pair_list with a target set size each -- and flip_batch turns a target into a margin from
the reference: the gap plus margin is put halfway between the two partial sums where the stop rule
has to fall, so every stopping test is as far from zero as the case allows.  For every compared
case the conditions under which a 1e-5 comparison of an fp64 device result is meaningful are
asserted here, none left out: cond(H - H_S) < 1e8, neighbouring sorted values further apart than
1e-7 of the largest, every stopping test further from zero than 1e-7 (|diff| + margin).  (1e-7 is
about 5 times the fp64 bound eps * COND_MAX = 2.2e-8 on a value's relative error.)"""
import ctypes
import functools
import types

import numpy as np
import pytest

from influence import _lib
from influence.NCF import NCF
from influence.matrix_factorization import MF

from test_abi import header_functions
from test_cand_newton_cpu import COND_MAX, params_for
from test_newton_cpu import DAMP, DUP, I, U, WD, _one_blas_thread, problem
from test_pair_cpu import SIZES, pair_list, pair_model, pair_reference

BAND = 1e-7
MAX_SET = 64          # the GPU test's batch; its second call uses 17
CF_MARGIN = 0.5       # the margin of the counterfactual-explanation cases


def flip_reference(model, p, k, tu, ti, tr, u, i, j, wd, damping, margin, max_set, ref=None):
    """The definition in numpy.  Returns dict(set_size, pos (positions in R_u), set_row, set_val,
    first_order, newton, dtheta, diff, cond (of H - H_S; NaN without a solve), sorted_val (every
    eligible value in selection order), partial (the running sums the stop rule tested), HS, bS,
    ref).  ref: pair_reference of (u, i, j), to share it between margins."""
    D3 = (3 * k + 3) if model == "MF" else 6 * k
    nan = dict(set_size=-1, pos=np.zeros(0, np.int64), set_row=np.zeros(0, np.int64), set_val=np.zeros(0),
               first_order=np.nan, newton=np.nan, dtheta=np.full(D3, np.nan), cond=np.nan, sorted_val=np.zeros(0),
               partial=[], ref=None)
    if not (0 <= u < U and 0 <= i < I and 0 <= j < I):
        return dict(nan, diff=np.nan)
    if i == j:
        return dict(nan, diff=0.0)
    if ref is None:
        ref = pair_reference(model, p, k, tu, ti, tr, u, i, j, wd, damping)
    n = ref["n"]
    if n == 0:
        return dict(nan, diff=ref["diff"], ref=ref)
    du = int((np.asarray(tu) == u).sum())
    rows, val = ref["rel"][:du], ref["influence"][:du]
    items = np.asarray(ti)[rows]
    elig = np.nonzero((items != i) & (items != j) & (val < 0.0))[0]          # ascending position
    order = elig[np.argsort(val[elig], kind="stable")]
    base = ref["diff"] + margin
    taken, s, partial = [], 0.0, []
    while len(taken) < max_set and len(taken) < order.size:
        partial.append(base + s)
        if not base + s >= 0.0:
            break
        s += val[order[len(taken)]]
        taken.append(order[len(taken)])
    else:
        if len(taken) < max_set:
            partial.append(base + s)                     # (the list ran out: the test that would have come)
    pos = np.array(taken, np.int64)
    out = dict(set_size=pos.size, pos=pos, set_row=rows[pos], set_val=val[pos], first_order=s if pos.size else 0.0,
               diff=ref["diff"], sorted_val=val[order], partial=partial, ref=ref)
    if not pos.size:
        return dict(out, newton=0.0, dtheta=np.zeros(D3), cond=np.nan, HS=np.zeros((D3, D3)), bS=np.zeros(D3))
    theta, M = pair_model(model, p, k, u, i, j)[:2]
    G, e = ref["G"][pos], ref["e"][pos]
    HS = (2.0 * G.T @ G + pos.size * wd * np.diag(M)) / n
    bS = (2.0 * e @ G + pos.size * wd * M * theta) / n
    with _one_blas_thread():
        dtheta = np.linalg.solve(ref["H"] - HS, bS)
        cond = float(np.linalg.cond(ref["H"] - HS))
    return dict(out, newton=float(ref["v"] @ dtheta), dtheta=dtheta, cond=cond, HS=HS, bS=bS)


def flip_cases(tu, ti):
    """(name, pair, target) of every case: pairs of pair_list (and one more one-rating user whose
    rating is not the pair's own) with what the margin is to bring about -- an int: exactly that
    many rows, flipping; "below": the gap is negative already, margin 0; "all": a margin no set
    closes, so rows are taken until the eligible ones or max_set run out; "zero": margin 0;
    a float: that margin; "disagree": the first size from which first order says flipped and the re-solved system says
    not (flip_batch searches it; None for a size that has none)."""
    pl = pair_list(tu, ti)
    heavy, heavy2, dup, user3, empty, one_own = pl[0], pl[8], pl[2], pl[3], pl[4], pl[9]
    assert heavy == (0, 7, 8) and dup[:2] == DUP and user3[0] == DUP[0] and empty[0] == 19 and one_own[0] == 17
    return [("below", None, "below"),                    # heavy or its swap, whichever gap is negative
            ("one", heavy, 1), ("few", heavy, 5), ("sixteen", heavy, 16), ("seventeen", heavy, 17),
            ("max_set", heavy, "all"),                   # user 0: more than 64 eligible rows
            ("exhausted", user3, "all"),                 # user 3: 36 ratings, about 20 negative values
            ("dup_own", dup, "all"),                     # (3, 5) sits in R_3 twice and is never taken
            ("empty_user", empty, "zero"), ("one_rating_own", one_own, "all"),
            ("one_rating", (17, 300, 301), "all"),
            ("other_heavy", heavy2, 3), ("unrated_j", pl[1], 2),
            ("disagree", heavy, "disagree"),
            # get_counterfactual_explanation's batch: user 0's test rating (0, 7) against three items
            ("cf_8", heavy, CF_MARGIN), ("cf_318", pl[1], CF_MARGIN), ("cf_40", (0, heavy[1], 40), CF_MARGIN)]


def _margin_for(ref_all, t):
    """The margin >= 0 that makes the set exactly t rows, flipping: diff + margin halfway between the
    lowest value the stop rule allows for t rows, max(diff, -S_(t-1)), and -S_t (S the cumulative
    sums of the sorted eligible values).  None: the pair cannot have such a set (too few eligible
    rows, or t rows do not close its gap even with margin 0)."""
    cum = np.concatenate([[0.0], np.cumsum(ref_all["sorted_val"])])
    if t >= cum.size or not ref_all["diff"] < -cum[t]:
        return None
    base = 0.5 * (max(ref_all["diff"], -cum[t - 1]) + -cum[t])
    return float(max(base - ref_all["diff"], 0.0))


@functools.lru_cache(maxsize=None)
def flip_batch(model, k):
    """The resolved cases of (model, k): list of dict(name, pair, margin, ref) with ref =
    flip_reference at MAX_SET; shared by the tests here and tests/test_gpu_flip.py (read-only)."""
    tu, ti, tr = problem()
    p = params_for(model, k)
    prs = {}

    def pref(q):
        if q not in prs:
            prs[q] = pair_reference(model, p, k, tu, ti, tr, q[0], q[1], q[2], WD, DAMP)
        return prs[q]

    def fr(q, margin, max_set=MAX_SET):
        return flip_reference(model, p, k, tu, ti, tr, q[0], q[1], q[2], WD, DAMP, margin, max_set, ref=pref(q))
    out = []
    for name, q, target in flip_cases(tu, ti):
        if target == "below":
            h = pair_list(tu, ti)[0]
            q = h if pref(h)["diff"] < 0.0 else (h[0], h[2], h[1])
            margin = 0.0
        elif target == "zero":
            margin = 0.0
        elif isinstance(target, float):
            margin = target
        elif target == "all":
            margin = 1e6
        elif target == "disagree":
            everything = fr(q, 1e6, 10 ** 6)
            margin = None
            for t in range(1, min(MAX_SET, everything["sorted_val"].size - 1) + 1):
                m = _margin_for(everything, t)
                if m is None:
                    continue
                r = fr(q, m)
                if r["set_size"] == t and r["diff"] + r["first_order"] < -m and not r["diff"] + r["newton"] < -m:
                    margin = m
                    break
            if margin is None:
                continue
        else:
            # the named pair, else its swap (the gap negated): the first that can have such a set
            for q in (q, (q[0], q[2], q[1])):
                margin = _margin_for(fr(q, 1e6, 10 ** 6), target)
                if margin is not None:
                    break
            assert margin is not None, (name, target)
        out.append(dict(name=name, pair=q, margin=margin, target=target, ref=fr(q, margin)))
    return out


@pytest.mark.parametrize("model,k", SIZES)
def test_cases_hold_what_the_gpu_test_needs(model, k):
    """The set sizes the issue's table asks for, and for EVERY compared case the conditioning, the
    distance between neighbouring sorted values and the distance of every stopping test from zero."""
    tu, ti, tr = problem()
    cases = {c["name"]: c for c in flip_batch(model, k)}
    size = lambda name: cases[name]["ref"]["set_size"]
    assert size("below") == 0 and cases["below"]["ref"]["diff"] < 0.0
    assert size("one") == 1 and 2 <= size("few") <= 8 and size("sixteen") == 16 and size("seventeen") == 17
    mx = cases["max_set"]["ref"]
    assert mx["set_size"] == MAX_SET and not mx["diff"] + mx["first_order"] < -cases["max_set"]["margin"]
    ex = cases["exhausted"]["ref"]
    assert 0 < ex["set_size"] == ex["sorted_val"].size < 36 and (tu == cases["exhausted"]["pair"][0]).sum() == 36
    dup_rows = np.nonzero((tu == DUP[0]) & (ti == DUP[1]))[0]
    assert dup_rows.size == 2 and not np.isin(dup_rows, cases["dup_own"]["ref"]["set_row"]).any()
    assert cases["dup_own"]["ref"]["set_size"] > 0
    assert size("empty_user") == 0 and cases["empty_user"]["ref"]["ref"]["n"] > 0
    assert size("one_rating_own") == 0 and (tu == 17).sum() == 1
    assert size("one_rating") in (0, 1) and size("other_heavy") == 3 and size("unrated_j") == 2
    for c in cases.values():
        r, margin = c["ref"], c["margin"]
        assert not isinstance(c["target"], int) or r["set_size"] == c["target"]
        if r["set_size"] > 0:
            assert r["cond"] < COND_MAX, (c["name"], r["cond"])
        first = r["sorted_val"][:r["set_size"] + 1]
        scale = np.abs(r["ref"]["influence"][:int((tu == c["pair"][0]).sum())]).max(initial=0.0)
        if first.size > 1:
            gap = np.diff(first).min()
            assert gap > BAND * scale, (c["name"], gap, scale)
        for t in r["partial"]:
            assert abs(t) > BAND * (abs(r["diff"]) + margin), (c["name"], t)
        # ... and the re-solved verdict diff + newton < -margin is not decided inside the 1e-5 the GPU
        # test allows newton (ten times that)
        if r["set_size"] > 0:
            assert abs(r["diff"] + r["newton"] + margin) > 1e-4 * abs(r["newton"]), (c["name"], r["newton"])
    worst = max(c["ref"]["cond"] for c in cases.values() if c["ref"]["set_size"] > 0)
    print("%s k=%d: sizes %s, largest cond(H - H_S) %.3e, disagree case: %s" % (
        model, k, {n: c["ref"]["set_size"] for n, c in cases.items()}, worst, "disagree" in cases))


@pytest.mark.parametrize("model", ["MF", "NCF"])
def test_first_order_and_newton_disagree_somewhere(model):
    """At least one case per model where first order says flipped and the re-solved system says not."""
    found = []
    for m, k in SIZES:
        if m != model:
            continue
        for c in flip_batch(m, k):
            if c["name"] == "disagree":
                r, mg = c["ref"], c["margin"]
                assert r["diff"] + r["first_order"] < -mg and not r["diff"] + r["newton"] < -mg
                found.append((k, r["set_size"], r["first_order"], r["newton"]))
    print(model, "disagreements (k, set size, first order, newton):", found)
    assert found


@pytest.mark.parametrize("model,k", SIZES)
def test_downdate_against_the_rebuilt_system(model, k):
    """H - H_S equals the H rebuilt row by row over rel without S's positions, keeping 1/n and with
    the decay scaled by (1 - |S| / n), to 1e-12 max|H|; x . b_S equals the summed values to 1e-12
    of the largest |val|."""
    tu, ti, tr = problem()
    p = params_for(model, k)
    checked = 0
    for c in flip_batch(model, k):
        r = c["ref"]
        if r["set_size"] <= 0 or c["name"] not in ("few", "seventeen", "exhausted", "dup_own"):
            continue
        u, i, j = c["pair"]
        pr = r["ref"]
        n = pr["n"]
        M, _, _, Ci, Cj = pair_model(model, p, k, u, i, j)[1:]
        keep = np.ones(n, bool)
        keep[r["pos"]] = False
        H = np.zeros_like(pr["H"])
        for pos in np.nonzero(keep)[0]:
            row = pr["rel"][pos]
            H += np.outer(pr["G"][pos], pr["G"][pos])
            if tu[row] == u and ti[row] == i:
                H += pr["e"][pos] * Ci
            if tu[row] == u and ti[row] == j:
                H += pr["e"][pos] * Cj
        H = (2.0 / n) * H + np.diag(WD * (1.0 - r["set_size"] / n) * M + DAMP)
        err = np.abs(H - (pr["H"] - r["HS"])).max() / np.abs(pr["H"]).max()
        e_fo = abs(pr["x"] @ r["bS"] - r["set_val"].sum()) / np.abs(r["set_val"]).max()
        print("%s k=%d %s: downdate %.2e, x . b_S against the summed values %.2e" % (model, k, c["name"], err, e_fo))
        assert err < 1e-12 and e_fo < 1e-12, (c["name"], err, e_fo)
        checked += 1
    assert checked == 4


def test_reference_edge_cases():
    tu, ti, tr = problem()
    p = params_for("MF", 8)
    for q, diff_nan in (((0, 7, 7), False), ((-1, 7, 8), True), ((0, 7, I), True), ((U, 7, 8), True)):
        r = flip_reference("MF", p, 8, tu, ti, tr, q[0], q[1], q[2], WD, DAMP, 0.0, 16)
        assert r["set_size"] == -1 and np.isnan(r["newton"]) and np.isnan(r["first_order"])
        assert np.isnan(r["dtheta"]).all() and (np.isnan(r["diff"]) if diff_nan else r["diff"] == 0.0)
    r = flip_reference("MF", p, 8, tu, ti, tr, 19, 318, 319, WD, DAMP, 0.0, 16)      # n == 0
    assert r["set_size"] == -1 and np.isfinite(r["diff"])
    # a smaller max_set cuts the same order
    big = flip_reference("MF", p, 8, tu, ti, tr, 0, 7, 8, WD, DAMP, 1e6, 64)
    small = flip_reference("MF", p, 8, tu, ti, tr, 0, 7, 8, WD, DAMP, 1e6, 17, ref=big["ref"])
    assert small["set_size"] == 17 and np.array_equal(small["set_row"], big["set_row"][:17])


# ------------------------------------------------------------------------------------------
# ABI and facade
# ------------------------------------------------------------------------------------------
def test_pair_flip_declared_exported_bound(libfia_path):
    assert "fia_pair_flip" in header_functions()
    assert hasattr(ctypes.CDLL(libfia_path), "fia_pair_flip")
    assert "fia_pair_flip" in _lib.SIGNATURES
    lib = _lib.load_library(libfia_path)
    assert lib.fia_pair_flip(None, 0, None, None, None, None, 16, None, None, None, None, None, None, None, None) == 1
    assert lib.fia_version() == 100
    assert _lib.FIA_FLIP_MAX_SET == 64
    from conftest import ROOT
    assert "#define FIA_FLIP_MAX_SET 64" in open(ROOT + "/include/fia.h").read()


@pytest.mark.parametrize("cls", [MF, NCF])
def test_flip_sets_host_validation(cls):
    m = cls.__new__(cls)          # no GPU context: only the host-side validation is exercised
    m.num_users, m.num_items, m.embedding_size, m.num_train_examples = 7, 5, 8, 20
    m.data_sets = {"test": types.SimpleNamespace(x=np.array([[0, 1], [3, 4]]))}
    for bad in ([2], [2, 3, 4], [2.5, 3.0], [-1, 3], [2, 5], [[2, 3]], [1, 3], [2, 4]):
        with pytest.raises(ValueError):
            m.get_flip_sets([0, 1], bad)
    for max_set in (0, -1, _lib.FIA_FLIP_MAX_SET + 1, 1.5, True):
        with pytest.raises(ValueError):
            m.get_flip_sets([0, 1], [2, 3], max_set=max_set)
    for margin in (-0.5, [0.1], [0.1, 0.2, 0.3], [0.1, -0.2], [0.1, np.nan], [[0.1, 0.2]]):
        with pytest.raises(ValueError):
            m.get_flip_sets([0, 1], [2, 3], margin=margin)
    for alts in ([], [[2, 3]]):
        with pytest.raises(ValueError):
            m.get_counterfactual_explanation(0, alts)
    with pytest.raises(ValueError):
        m.get_counterfactual_explanation(0, [2, 1])            # an alternative is the own item
    mg, ms = m._checked_flip_args(2, 0.25, 64)
    assert mg.tolist() == [0.25, 0.25] and ms == 64 and m._checked_flip_args(2, None, 1) == (None, 1)
