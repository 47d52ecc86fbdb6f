"""Oracle tests of the MF k = 16 query path whose chunk scan and side-system solves are one
launch (k_solve_quad: workgroups [0, tiles) run the scan, the others eight solve waves of 8
queries each) and whose coupled-query list is emptied by the coupled solve's last reader.

Every comparison is against the fp64 oracle (oracle.fia_oracle) through the helpers of the
existing suites: related sets bit-exact, influence and x < RTOL, top-1 by check_topk's tie
rule.  One small problem serves every test: 600 x 40 entities, 701 ratings, wd = 1e-3,
damping = 1e-6, parameters from synth.mf_params; the oracle's answer is computed once per
distinct (user, item) pair and shared read-only."""
import numpy as np
import pytest

from influence import synth
from test_gpu_mfma_score import RawModel, WD, DAMPING, bits, check_against_oracle
from test_gpu_parity import RTOL, rel_err

pytestmark = pytest.mark.gpu

K16 = 16
U, I, N0 = 600, 40, 700
_STATE = {}


def problem():
    """Users 0 .. U-2 x items 0 .. I-2 hold N0 distinct ratings, and row 5's pair once more (a
    pair present twice in train); user U-1 and item I-1 have empty lists.  The train rows are
    permuted, so list order is train-row order and not id order."""
    if "p" not in _STATE:
        rng = np.random.default_rng(1916)
        key = rng.choice((U - 1) * (I - 1), N0, replace=False)
        tu, ti = (key // (I - 1)).astype(np.int32), (key % (I - 1)).astype(np.int32)
        tu, ti = np.append(tu, tu[5]), np.append(ti, ti[5])
        perm = rng.permutation(tu.size)
        tu, ti = tu[perm], ti[perm]
        tr = rng.integers(1, 6, tu.size).astype(np.float32)
        p = synth.mf_params(U, I, K16, 11)
        train_pairs = sorted(set(zip(tu.tolist(), ti.tolist())))
        twice = (int(key[5] // (I - 1)), int(key[5] % (I - 1)))
        assert sum(1 for a, b in zip(tu, ti) if (a, b) == twice) == 2
        have = set(train_pairs)
        free = []
        while len(free) < 240:
            u, i = int(rng.integers(0, U - 1)), int(rng.integers(0, I - 1))
            if (u, i) not in have:
                free.append((u, i))
        _STATE["p"] = dict(train=(tu, ti, tr), params=p, train_pairs=train_pairs, twice=twice, free=free)
    return _STATE["p"]


def oracle_for(qu, qi):
    """The oracle's result per query (memoised per pair); an id out of range is the empty
    query: no related ratings, NaN x (include/fia.h: never used as an index)."""
    from oracle import fia_oracle as fo
    P = problem()
    if "ex" not in _STATE:
        tu, ti, tr = P["train"]
        _STATE["ex"] = fo.CsrExact("MF", P["params"], K16, tu, ti, tr, WD, DAMPING)
        _STATE["memo"] = {}
    memo, out = _STATE["memo"], []
    for u, i in zip(qu.tolist(), qi.tolist()):
        if (u, i) not in memo:
            if 0 <= u < U and 0 <= i < I:
                memo[(u, i)] = _STATE["ex"].query(u, i)
            else:
                memo[(u, i)] = dict(rel=np.zeros(0, np.int64), n=0, influence=np.zeros(0),
                                    x=np.full(2 * K16 + 2, np.nan))
        out.append(memo[(u, i)])
    return out


def model():
    P = problem()
    return RawModel("MF", K16, U, I, P["train"], P["params"])


def by_item(pairs):
    """Queries sorted by item (the item runs of the scoring kernel), stable."""
    qu = np.array([q[0] for q in pairs], np.int32)
    qi = np.array([q[1] for q in pairs], np.int32)
    order = np.argsort(qi, kind="stable")
    return qu[order], qi[order]


def draw(rng, Q, n_coupled=0):
    P = problem()
    pairs = [P["free"][j] for j in rng.integers(0, len(P["free"]), Q - n_coupled)]
    pairs += [P["train_pairs"][j] for j in rng.integers(0, len(P["train_pairs"]), n_coupled)]
    return by_item(pairs)


def run(m, qu, qi, K=1, want_x=True, want_rel=True, want_infl=True, x_in=None, checked=True):
    """count (host-checked unless `checked` is False: out-of-range ids are refused there) and one
    fia_query_batch / fia_query_batch_x; every output the call was given, as numpy."""
    t = m.torch
    dqu, dqi = m.dev_queries(qu, qi)
    if checked:
        off, tot = m.ctx.count_related(dqu, dqi)
    else:
        off, _ = m.ctx.count_related(dqu, dqi, want_total=False)
        tot = int(off[-1].item())
    Q, D = len(qu), m.ctx.num_params()
    rel = t.full((max(tot, 1),), -7, dtype=t.int32, device=m.dev) if want_rel else None
    infl = t.full((max(tot, 1),), float("nan"), dtype=t.float64, device=m.dev) if want_infl else None
    x = t.zeros(Q * D, dtype=t.float64, device=m.dev) if want_x and x_in is None else None
    tp = t.zeros(max(Q * K, 1), dtype=t.int64, device=m.dev) if K else None
    tix = t.zeros(max(Q * K, 1), dtype=t.int64, device=m.dev) if K else None
    tv = t.zeros(max(Q * K, 1), dtype=t.float64, device=m.dev) if K else None
    if x_in is None:
        m.ctx.query_batch(dqu, dqi, off, tot, rel, infl, x, K, tp, tix, tv)
    else:
        m.ctx.query_batch_x(dqu, dqi, off, tot, x_in, rel, infl, K, tp, tix, tv)
    t.cuda.synchronize(m.dev)
    out = dict(offsets=off.cpu().numpy())
    if want_rel:
        out["rel_idx"] = rel[:tot].cpu().numpy().astype(np.int64)
    if want_infl:
        out["influence"] = infl[:tot].cpu().numpy()
    if x is not None:
        out["x"] = x.cpu().numpy().reshape(Q, D)
    if K:
        out.update(topk_pos=tp.cpu().numpy().reshape(Q, K), topk_idx=tix.cpu().numpy().reshape(Q, K),
                   topk_val=tv.cpu().numpy().reshape(Q, K))
    return out


def same_bits(a, b, names=None):
    for name in (names or a):
        x, y = a[name], b[name]
        if x.dtype == np.float64:
            assert np.array_equal(bits(x), bits(y)), name
        else:
            assert np.array_equal(x, y), name


# ---------------------------------------------------------------------------------------
# 1. role boundaries
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("Q", [1, 7, 8, 9, 63, 64, 65, 511, 512, 513, 1025])
def test_role_boundaries(Q):
    """Batch sizes across the quad / wave (8 queries) / solve workgroup (64) edges of the solve
    role and the 512-entry tile edge of the scan role (the scan covers Q + 1 entries: 511 is
    one tile, 512 two, 1025 three), a twentieth of the queries coupled."""
    rng = np.random.default_rng(1000 + Q)
    qu, qi = draw(rng, Q, n_coupled=Q // 20)
    m = model()
    res = run(m, qu, qi, K=1)
    check_against_oracle(res, oracle_for(qu, qi), 1, "role boundary Q=%d" % Q)
    m.close()


# ---------------------------------------------------------------------------------------
# 2. coupled pairs (the test pair is a train row)
# ---------------------------------------------------------------------------------------
def coupled_case(case):
    P = problem()
    rng = np.random.default_rng(77)
    Q = 70                                              # two solve workgroups
    free = [P["free"][j] for j in rng.choice(len(P["free"]), Q, replace=False)]
    cpl = [P["train_pairs"][j] for j in rng.choice(len(P["train_pairs"]), Q, replace=False)]
    if case == "none":
        pairs = free
    elif case == "one":
        pairs = free[:40] + cpl[:1] + free[41:]
    elif case == "several":
        pairs = free[:]
        for j in (3, 8, 9, 31, 63, 64, 66):
            pairs[j] = cpl[j]
    elif case == "all":
        pairs = cpl
    elif case == "first-and-last":
        pairs = cpl[:1] + free[1:-1] + cpl[1:2]
    else:                                               # the pair present twice in train
        pairs = free[:20] + [P["twice"]] + free[21:]
    if case == "first-and-last":
        # keep the batch order: the coupled queries are first and last as given
        qu = np.array([q[0] for q in pairs], np.int32)
        qi = np.array([q[1] for q in pairs], np.int32)
        have = set(P["train_pairs"])
        assert (qu[0], qi[0]) in have and (qu[-1], qi[-1]) in have
        return qu, qi
    return by_item(pairs)


@pytest.mark.parametrize("case", ["none", "one", "several", "all", "first-and-last", "twice-in-train"])
def test_coupled_pairs(case):
    """The coupled list and its count: filled by the solve role, read and emptied by the
    coupled solve.  The same context answers the batch twice (the second call finds what the
    first left) with the same bits."""
    qu, qi = coupled_case(case)
    have = set(problem()["train_pairs"])
    n_cpl = sum((int(u), int(i)) in have for u, i in zip(qu, qi))
    assert n_cpl == dict(none=0, one=1, several=7, all=70).get(case, 2 if case == "first-and-last" else 1)
    m = model()
    want = oracle_for(qu, qi)
    first = run(m, qu, qi, K=1)
    check_against_oracle(first, want, 1, "coupled %s" % case)
    again = run(m, qu, qi, K=1)
    same_bits(first, again)
    m.close()


# ---------------------------------------------------------------------------------------
# 3. degenerate queries inside a normal batch
# ---------------------------------------------------------------------------------------
def test_degenerate_queries():
    """Ids out of range (never used as an index: no ratings, NaN x) and a user and an item
    with empty lists (n = 0: NaN record and NaN x) among ordinary and coupled queries."""
    P = problem()
    rng = np.random.default_rng(5)
    pairs = [P["free"][j] for j in rng.choice(len(P["free"]), 80, replace=False)]
    pairs[0] = (-1, 3)
    pairs[7] = (U, 4)
    pairs[8] = (5, I)
    pairs[40] = (2, -3)
    pairs[63] = (U - 1, I - 1)                          # both lists empty
    pairs[64] = (1 << 30, 1 << 30)
    pairs[70] = P["train_pairs"][9]
    pairs[79] = (U - 1, I - 1)
    qu = np.array([q[0] for q in pairs], np.int32)
    qi = np.array([q[1] for q in pairs], np.int32)
    want = oracle_for(qu, qi)
    assert sum(o["n"] == 0 for o in want) == 7
    m = model()
    for K in (0, 1):
        res = run(m, qu, qi, K=K, checked=False)
        check_against_oracle(res, want, K, "degenerate K=%d" % K)
    m.close()


# ---------------------------------------------------------------------------------------
# 4. state left clean
# ---------------------------------------------------------------------------------------
def test_state_left_clean():
    """One context answers batches of 513, 7, 1025 and 64 queries in turn, with and without
    coupled pairs, a fia_query_batch_x call (the scan as a launch of its own, no solve) and a
    bare fia_count_related in between; every call matches the oracle; the whole sequence twice
    gives the same bits."""
    m = model()
    rounds = []
    for rnd in range(2):
        rng = np.random.default_rng(31)
        outs = []
        for Q, n_cpl in ((513, 30), (7, 0), (1025, 0), (64, 64), (1025, 90), (7, 3), (513, 0), (64, 0)):
            qu, qi = draw(rng, Q, n_coupled=n_cpl)
            want = oracle_for(qu, qi)
            res = run(m, qu, qi, K=1)
            check_against_oracle(res, want, 1, "sequence %d Q=%d coupled=%d" % (rnd, Q, n_cpl))
            outs.append(res)
            # the given-x call on another batch size: x of a fresh solve, so its influence is
            # the oracle's too
            qu2, qi2 = draw(rng, 100, n_coupled=10)
            x = run(m, qu2, qi2, K=0)["x"]
            x_in = m.torch.from_numpy(np.ascontiguousarray(x.reshape(-1))).to(m.dev)
            given = run(m, qu2, qi2, K=1, x_in=x_in)
            want2 = oracle_for(qu2, qi2)
            for q, o in enumerate(want2):
                b, e = given["offsets"][q], given["offsets"][q + 1]
                assert np.array_equal(given["rel_idx"][b:e], o["rel"]), (rnd, Q, q)
                assert rel_err(given["influence"][b:e], o["influence"]) < RTOL, (rnd, Q, q)
            outs.append(given)
            dqu, dqi = m.dev_queries(qu, qi)
            off, tot = m.ctx.count_related(dqu, dqi)
            assert tot == sum(o["n"] for o in want) and np.array_equal(off.cpu().numpy(), res["offsets"])
        rounds.append(outs)
    for a, b in zip(*rounds):
        same_bits(a, b)
    m.close()


# ---------------------------------------------------------------------------------------
# 5. output options
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [0, 1])
def test_output_options(K):
    """x_out given and NULL, rel_idx / influence NULL, with and without the top-1: whatever
    is given equals the all-outputs run bit for bit, and that run matches the oracle."""
    rng = np.random.default_rng(8)
    qu, qi = draw(rng, 130, n_coupled=9)
    m = model()
    full = run(m, qu, qi, K=K)
    check_against_oracle(full, oracle_for(qu, qi), K, "outputs K=%d" % K)
    for want_x in (True, False):
        for want_rel, want_infl in ((True, True), (False, True), (True, False), (False, False)):
            if not K and not want_rel and not want_infl and not want_x:
                continue                                # nothing asked for
            part = run(m, qu, qi, K=K, want_x=want_x, want_rel=want_rel, want_infl=want_infl)
            same_bits(part, full, names=list(part))
    m.close()


# ---------------------------------------------------------------------------------------
# 6. two contexts on two streams
# ---------------------------------------------------------------------------------------
def test_two_contexts_two_streams():
    """Two contexts answer different batches on two streams with nothing between their calls
    (two batches in flight): each equals its own serial answer bit for bit, and that answer
    matches the oracle."""
    import torch
    rng = np.random.default_rng(99)
    batches = [draw(rng, 513, n_coupled=25), draw(rng, 700, n_coupled=0)]
    ms = [model(), model()]
    dev = ms[0].dev
    serial, args = [], []
    for m, (qu, qi) in zip(ms, batches):
        res = run(m, qu, qi, K=1)
        check_against_oracle(res, oracle_for(qu, qi), 1, "serial Q=%d" % len(qu))
        serial.append(res)
    streams = [torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)]
    for m, (qu, qi), s, res in zip(ms, batches, streams, serial):
        with torch.cuda.stream(s):
            dqu, dqi = m.dev_queries(qu, qi)
            off = torch.from_numpy(res["offsets"]).to(dev)
            tot, Q, D = int(res["offsets"][-1]), len(qu), m.ctx.num_params()
            args.append(dict(dqu=dqu, dqi=dqi, off=off, tot=tot,
                             rel=torch.zeros(tot, dtype=torch.int32, device=dev),
                             infl=torch.zeros(tot, dtype=torch.float64, device=dev),
                             x=torch.zeros(Q * D, dtype=torch.float64, device=dev),
                             tp=torch.zeros(Q, dtype=torch.int64, device=dev),
                             tix=torch.zeros(Q, dtype=torch.int64, device=dev),
                             tv=torch.zeros(Q, dtype=torch.float64, device=dev)))
    torch.cuda.synchronize(dev)
    for _ in range(4):                                  # the first round moves each context to its stream
        for m, s, a in zip(ms, streams, args):
            with torch.cuda.stream(s):
                m.ctx.prepare()
                m.ctx.count_related(a["dqu"], a["dqi"], a["off"], want_total=False)
                m.ctx.query_batch(a["dqu"], a["dqi"], a["off"], a["tot"], a["rel"], a["infl"], a["x"], 1,
                                  a["tp"], a["tix"], a["tv"])
    torch.cuda.synchronize(dev)
    for a, res, (qu, qi) in zip(args, serial, batches):
        Q = len(qu)
        got = dict(offsets=a["off"].cpu().numpy(), rel_idx=a["rel"].cpu().numpy().astype(np.int64),
                   influence=a["infl"].cpu().numpy(), x=a["x"].cpu().numpy().reshape(Q, -1),
                   topk_pos=a["tp"].cpu().numpy().reshape(Q, 1), topk_idx=a["tix"].cpu().numpy().reshape(Q, 1),
                   topk_val=a["tv"].cpu().numpy().reshape(Q, 1))
        same_bits(got, res)
    for m in ms:
        m.close()
