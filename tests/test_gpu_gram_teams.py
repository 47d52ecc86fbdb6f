"""The MF k <= 16 Gram stream with team workgroups (k_gram_mf_stream, build_gram_stream): a
list of 2 .. TEAM_REACH slices of GS_SLICE ratings is summed in LDS by the one workgroup that
holds all of its slices; a longer list still writes partial Grams that k_gram_combine sums.
One small problem whose item list lengths form a ladder around every edge of that schedule,
at k = 8 and k = 16.

Every comparison is against the fp64 oracle (oracle.fia_oracle) unless it says bitwise: related
sets bit-exact, influence and x < RTOL, top-1 by check_topk (check_against_oracle does all
three for every query of the batch).  wd = 1e-3, damping = 1e-6, parameters from
synth.mf_params.

The schedule the cases rely on (build_gram_stream): teams come first, longest first, both sides
merged, each in consecutive waves of one 4-wave workgroup (one slice per wave up to 4 slices,
then ceil(slices / 4) per wave); a team that does not fit behind the last one opens a new
workgroup.  Here: {3072}, {1025: 3 waves}, {1024}, {513: 3 waves}, {512, user LONG_USER},
{257}; the free waves take the slices of the 4100- and the 3073-list and then the whole
lists."""
import numpy as np
import pytest

from influence import synth
from test_gpu_mfma_score import RawModel, WD, DAMPING, check_against_oracle, oracle_results
from test_gpu_parity import RTOL, rel_err
from test_gpu_scan_solve import same_bits

GS_SLICE = 256                 # kGsSlice: ratings per Gram-stream slice
GS_WAVES = 4                   # kGsWaves: waves of a workgroup
TEAM_REACH = 12                # kGsTeamSlices: most slices of a list summed by its workgroup
LADDER = [0, 1, 16, 17, 255, 256, 257, 512, 513, 1024, 1025, 3072, 3073, 4100]
LONG_USER_LEN = 300
U, I = 4200, 320
LONG_USER = U - 1
KS = [8, 16]
_STATE = {}


def slices(n):
    return max(1, -(-n // GS_SLICE))


def test_ladder_straddles_the_schedule_edges():
    """The ladder has a list at and beside every edge the constants above set (no GPU)."""
    ns = [slices(n) for n in LADDER]
    assert GS_SLICE in LADDER and GS_SLICE - 1 in LADDER and GS_SLICE + 1 in LADDER
    assert 2 * GS_SLICE in LADDER and 2 * GS_SLICE + 1 in LADDER
    assert GS_WAVES * GS_SLICE in LADDER and GS_WAVES * GS_SLICE + 1 in LADDER      # 4 and 5 slices
    assert TEAM_REACH * GS_SLICE in LADDER and TEAM_REACH * GS_SLICE + 1 in LADDER  # 12 and 13 slices
    assert max(ns) > TEAM_REACH + 1 and 1 in ns and 2 in ns and 3 in ns
    assert 1 < slices(LONG_USER_LEN) <= GS_WAVES
    assert max(LADDER) < U - 1 and LONG_USER_LEN < I - len(LADDER)


def problem():
    """Item j < len(LADDER) has LADDER[j] raters among users 0 .. U-2; user LONG_USER rates
    LONG_USER_LEN of the other items (one rating each from it), and those items get a few more
    raters.  Train rows are permuted: list order is train-row order, not id order."""
    if "p" not in _STATE:
        rng = np.random.default_rng(2024)
        L = len(LADDER)
        us, its = [], []
        for j, n in enumerate(LADDER):
            us.append(rng.choice(U - 1, n, replace=False))
            its.append(np.full(n, j))
        long_items = L + rng.choice(I - L, LONG_USER_LEN, replace=False)
        us.append(np.full(LONG_USER_LEN, LONG_USER))
        its.append(long_items)
        for j in range(L, I):
            r = rng.choice(U - 1, 3 + j % 4, replace=False)
            us.append(r)
            its.append(np.full(r.size, j))
        tu = np.concatenate(us).astype(np.int32)
        ti = np.concatenate(its).astype(np.int32)
        perm = rng.permutation(tu.size)
        tu, ti = tu[perm], ti[perm]
        tr = rng.integers(1, 6, tu.size).astype(np.float32)
        assert tu.size < 20000
        deg_u, deg_i = np.bincount(tu, minlength=U), np.bincount(ti, minlength=I)
        assert list(deg_i[:L]) == LADDER and deg_u[LONG_USER] == LONG_USER_LEN
        assert deg_u[:U - 1].max() <= GS_SLICE and deg_i[L:].max() <= GS_SLICE   # no other split list
        # every ladder item with a short-list user (a rater of it where it has one: that pair is a
        # train row; else any user with ratings), the long user with a short item it did not rate
        qs = []
        for j, n in enumerate(LADDER):
            raters = tu[ti == j]
            qs.append((int(raters[0]) if n and j % 2 else int(np.nonzero(deg_u[:U - 1] > 0)[0][j]), j))
        short_item = int(np.setdiff1d(np.arange(L, I), long_items)[0])
        qs.append((LONG_USER, short_item))
        qu = np.array([q[0] for q in qs], np.int32)
        qi = np.array([q[1] for q in qs], np.int32)
        assert (deg_u[qu[:-1]] < 16).all() and 0 < deg_i[short_item] < 16
        _STATE["p"] = dict(train=(tu, ti, tr), qu=qu, qi=qi, deg_u=deg_u, deg_i=deg_i,
                           params={k: synth.mf_params(U, I, k, 17) for k in KS})
    return _STATE["p"]


def want_for(k):
    P = problem()
    return oracle_results(("gram-teams", k), k, P["params"][k], P["train"], P["qu"], P["qi"])


def item_q(n):
    return LADDER.index(n)


@pytest.mark.parametrize("k", KS)
def test_oracle_is_settled_on_the_ladder(k):
    """The tolerance tests the kernel, not the problem's conditioning (no GPU): the oracle's
    answers are finite, and its two implementations (fia_oracle.query, dense; CsrExact) agree far
    below RTOL on the queries of the longest lists, the long user and a short list."""
    from oracle import fia_oracle as fo
    P = problem()
    tu, ti, tr = P["train"]
    want = want_for(k)
    for o in want:
        assert np.isfinite(o["influence"]).all() and (o["n"] == 0 or np.isfinite(o["x"]).all())
    for q in (item_q(4100), item_q(3072), item_q(257), item_q(16), len(LADDER)):
        o = fo.query("MF", P["params"][k], k, tu, ti, tr, int(P["qu"][q]), int(P["qi"][q]), WD, DAMPING)
        assert np.array_equal(o["rel"], want[q]["rel"])
        ei, ex = rel_err(o["influence"], want[q]["influence"]), rel_err(o["x"], want[q]["x"])
        assert ei < 1e-4 * RTOL and ex < 1e-4 * RTOL, (k, q, ei, ex)


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
def test_every_ladder_list_matches_the_oracle(k):
    """Case 1: every query of the batch -- each ladder item with a short-list user, the
    300-rating user with a short item -- against CsrExact: related set, x, influence, top-1."""
    P = problem()
    m = RawModel("MF", k, U, I, P["train"], P["params"][k])
    res = m.batch(P["qu"], P["qi"], 1)
    want = want_for(k)
    assert all(o["n"] >= n for o, n in zip(want, LADDER)) and want[-1]["n"] >= LONG_USER_LEN
    check_against_oracle(res, want, 1, "gram teams k=%d" % k)
    m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
def test_same_bits_again_and_on_a_fresh_context(k):
    """Case 2: the same batch twice on one context (the second after a second full prepare), and
    once on a fresh context: the same bits."""
    P = problem()
    m = RawModel("MF", k, U, I, P["train"], P["params"][k])
    a = m.batch(P["qu"], P["qi"], 1)
    m.ctx.prepare()
    b = m.batch(P["qu"], P["qi"], 1)
    m.close()
    m2 = RawModel("MF", k, U, I, P["train"], P["params"][k])
    c = m2.batch(P["qu"], P["qi"], 1)
    m2.close()
    same_bits(a, b)
    same_bits(a, c)


SUBSETS = {
    # the 512-item's team shares its workgroup with the long user's team: the item is marked
    # (with its short-list user), the long user is not
    "team-beside-unmarked-team": [item_q(512)],
    # and the other way round
    "unmarked-team-beside-team": [len(LADDER)],
    # only the lists past the reach (partial slots + k_gram_combine) and their short users
    "past-the-reach-only": [item_q(3073), item_q(4100)],
    # only whole short lists: every team and every combine entry is skipped
    "whole-lists-only": [item_q(0), item_q(1), item_q(17), item_q(255), item_q(256)],
    # teams of every depth, the other teams unmarked
    "some-teams": [item_q(257), item_q(1025), item_q(3072)],
}


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("subset", sorted(SUBSETS))
def test_prepare_for_subsets_match_the_full_prepare(k, subset):
    """Case 3: a context whose only prepare is fia_prepare_for of a subset gives the covered
    queries the bits of the full prepare (and so the oracle's answer, by case 1)."""
    P = problem()
    if ("full", k) not in _STATE:
        m = RawModel("MF", k, U, I, P["train"], P["params"][k])
        _STATE[("full", k)] = m.batch(P["qu"], P["qi"], 1)
        m.close()
    full = _STATE[("full", k)]
    sel = np.array(SUBSETS[subset])
    qu, qi = P["qu"][sel], P["qi"][sel]
    if subset == "team-beside-unmarked-team":
        assert LONG_USER not in qu
    if subset == "past-the-reach-only":
        assert all(slices(int(P["deg_i"][i])) > TEAM_REACH for i in qi)
    if subset == "whole-lists-only":
        assert all(P["deg_i"][i] <= GS_SLICE for i in qi)
    m = RawModel("MF", k, U, I, P["train"], P["params"][k], prepare=False)
    m.prepare_for(qu, qi)
    part = m.batch(qu, qi, 1)
    m.close()
    offs = full["offsets"]
    for t, q in enumerate(sel):
        b, e = offs[q], offs[q + 1]
        pb, pe = part["offsets"][t], part["offsets"][t + 1]
        assert pe - pb == e - b
        got = dict(rel_idx=part["rel_idx"][pb:pe], influence=part["influence"][pb:pe], x=part["x"][t],
                   topk_pos=part["topk_pos"][t], topk_idx=part["topk_idx"][t], topk_val=part["topk_val"][t])
        ref = dict(rel_idx=full["rel_idx"][b:e], influence=full["influence"][b:e], x=full["x"][q],
                   topk_pos=full["topk_pos"][q], topk_idx=full["topk_idx"][q], topk_val=full["topk_val"][q])
        same_bits(got, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
def test_second_index_without_split_lists(k):
    """Case 4: on the context that has prepared the ladder, a second index without any split
    list (no team, no partial slot, no combine entry): the cached schedule is rebuilt for it and
    nothing of the first index's is used.  Against the oracle."""
    import torch
    P = problem()
    m = RawModel("MF", k, U, I, P["train"], P["params"][k])
    m.batch(P["qu"], P["qi"], 1)
    rng = np.random.default_rng(77)
    N2 = 6000
    key = np.sort(rng.choice(U * I, N2, replace=False))
    tu, ti = (key // I).astype(np.int32), (key % I).astype(np.int32)
    tr = rng.integers(1, 6, N2).astype(np.float32)
    assert np.bincount(tu, minlength=U).max() <= GS_SLICE and np.bincount(ti, minlength=I).max() <= GS_SLICE
    m.train = [torch.from_numpy(a).to(m.dev) for a in (tu, ti, tr)]
    m.ctx.build_index(m.train[0], m.train[1], m.train[2], U, I)
    m.ctx.prepare()
    qu, qi = P["qu"], P["qi"]
    res = m.batch(qu, qi, 1)
    want = oracle_results(("gram-teams-second", k), k, P["params"][k], (tu, ti, tr), qu, qi)
    check_against_oracle(res, want, 1, "second index k=%d" % k)
    m.close()
