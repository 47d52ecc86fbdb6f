"""The yardstick of test_gpu_accuracy.py, validated without a GPU before any kernel is judged
by it (tests/accuracy_problems.py: problems, longdouble reference, derived bounds).

Per (configuration, regime) -- every regime at the small-k configurations, `base` and
`nodecay` at the two large-k ones (a sample: their references are the slow ones):
  (a) headroom: a plain fp64 numpy pipeline (Gram summed in list order, unpivoted LDL^T in the
      library's block order) stays within bound / 16 on every asserted system, and its scoring
      within bound / 16 of the longdouble scoring of the same x;
  (b) the regime reaches what it claims (below);
  (c) every uncoupled query with n > 0 is asserted (>= 90 % is the floor the design sets), and
      `base` and `small` assert at least one coupled query;
  (d) rho and eta of the coupled queries are printed, and asserted only against the
      growth-aware bound.
The longdouble restatement is also compared with oracle/fia_oracle.py (its fp64 H, v, related
lists), so the yardstick and the existing oracle describe the same systems.

(b) as measured on these problems, largest cond of an uncoupled side block per regime:
  MF   base 6e3 - 8e3,  nodecay 3.5e9 - 4.0e9,  big 5.4e8 - 8.4e8
  NCF  base 36 - 214,   nodecay 3.5e7 - 2.1e8,  big 1.5e4 - 1.5e5
MF meets cond >= 1e8 (`nodecay`) and >= 1e7 (`big`) at every k.  NCF cannot: every NCF
parameter is decayed, so the floor of a block is wd + damping = 1.001e-3 in `big`, and the
gradients are O(1 / k), which puts the largest eigenvalue of a rank-deficient block at about
0.1 (k = 16) to 0.035 (k = 64) over the floor 1e-9 of `nodecay`.  NCF is therefore held to
what the regimes do to its blocks by construction: `nodecay` lowers the floor by
1.001e-3 / 1e-9 (asserted: >= 1e5 x the `base` cond, and >= 1e8 itself at k <= 16), `big`
scales the GMF half of every gradient by 30 (asserted: >= 100 x the `base` cond; 300 - 700 x
measured)."""
import numpy as np
import pytest

import accuracy_problems as ap

SMALL_K = [c for c in ap.CONFIGS if c not in ap.LARGE_K]
CASES = [(c, r) for c in SMALL_K for r in ap.REGIMES] + [(c, r) for c in ap.LARGE_K for r in ("base", "nodecay")]
HEADROOM = 16.0


def case_id(v):
    return ap.config_id(v)


def side_conds(ref):
    """Largest 2-norm condition number over the side blocks of the uncoupled queries."""
    worst = 0.0
    for q in range(ref.qu.size):
        for name, sl, H, v, b, rho in ap.systems(ref, q):
            if name != "coupled":
                worst = max(worst, float(np.linalg.cond(H.astype(np.float64))))
    return worst


@pytest.mark.parametrize("cfg,regime", CASES, ids=case_id)
def test_yardstick(cfg, regime):
    from oracle import fia_oracle as fo
    model, k = cfg
    assert np.finfo(ap.LD).eps < 1e-18
    ap.assert_problem_claims(model, k)
    ref = ap.reference(model, k, regime)
    p64 = ap.Reference(model, k, regime, np.float64)
    lo = ap.lib_order(model, k)
    Q = ref.qu.size

    # the restatement describes the oracle's systems
    ex = fo.CsrExact(model, ref.params, k, ref.train[0], ref.train[1], ref.train[2], ref.wd, ref.damping)
    for q in range(Q):
        s = ref.system(q)
        o = ex.query(s["u"], s["i"])
        assert np.array_equal(o["rel"], ref.related(s["u"], s["i"])) and o["n"] == s["n"]
        assert np.abs(o["v"][lo] - s["v"].astype(np.float64)).max() <= 1e-13 * np.abs(o["v"]).max()
        if s["n"]:
            Ho = o["H"][np.ix_(lo, lo)]
            assert np.abs(Ho - s["H"].astype(np.float64)).max() <= 1e-12 * np.abs(Ho).max(), q

    # (a) the fp64 pipeline, system by system
    def x64(q):
        s = p64.system(q)
        if s["coupled"]:
            return ap.ldlt_solve(s["H"].copy(), s["v"].copy())
        Ds = ref.Ds
        return np.concatenate([ap.ldlt_solve(s["H"][sl, sl].copy(), s["v"][sl].copy())
                               for sl in (slice(0, Ds), slice(Ds, 2 * Ds))])
    recs = ap.judge(ref, x64)
    for q, name, e, b, rho in recs:
        if b is not None:
            assert e <= b / HEADROOM, (model, k, regime, q, name, e, b)
            assert name == "coupled" or b <= ap.UNCOUPLED_CAP
    for q in range(Q):
        if ref.system(q)["n"]:
            x = x64(q)
            want, bound = ref.influence(q, x)
            got, _ = p64.influence(q, x)
            assert (np.abs(got.astype(ap.LD) - want) <= bound / HEADROOM).all(), (model, k, regime, q)

    # (c) what is asserted
    uncoupled = [q for q in range(Q) if ref.kinds[q] not in ("rater", "twice")]
    judged = {q for q, name, e, b, rho in recs if name != "coupled" and b is not None}
    with_n = [q for q in uncoupled if ref.system(q)["n"] > 0]
    assert [q for q in uncoupled if q not in with_n] == [ref.kinds.index("none")]
    assert judged == set(with_n) and len(judged) >= 0.9 * len(uncoupled)
    sm = ap.summary(recs)
    if regime in ("base", "small"):
        assert sm["coupled_asserted"] >= 1
    for key in ap.CLAMPED:                         # the one place the derived bound is over the cap
        pr = ap.problem("MF", 64)
        assert key[:3] == ("MF", 64, "big") and key[4] == "item" and pr[6][pr[4][key[3]]] == 4100, key

    # (b) what the regime reaches
    cond = side_conds(ref)
    if regime in ("nodecay", "big"):
        base = side_conds(ap.reference(model, k, "base"))
        if model == "MF":
            assert cond >= (1e8 if regime == "nodecay" else 1e7), cond
        elif regime == "nodecay":
            assert cond >= 1e5 * base and (k > 16 or cond >= 1e8), (cond, base)
        else:
            assert cond >= 100 * base, (cond, base)
    if regime == "collinear":
        ratios = []
        for n in (ref.Ds + 1, 300):
            sv = np.linalg.svd(ref.entity(1, ref.lengths.index(n)).A.astype(np.float64), compute_uv=False)
            ratios.append(sv[1] / sv[0])
        print("collinear %s k=%d: Gram sigma2 / sigma1 %s" % (model, k, ["%.1e" % r for r in ratios]))
        assert min(ratios) < 1e-6, ratios
    if regime == "base":
        assert max(rho for q, name, e, b, rho in recs if name == "coupled") > 10

    # (d) the growth record
    print("%s k=%d %s: side cond %.1e | fp64 numpy: side eta %.1e / bound %.1e, coupled eta %.1e / bound %.1e "
          "(%d asserted), rho max %.1e, %d over the cap with eta up to %.1e"
          % (model, k, regime, cond, sm["side_eta"], sm["side_bound"], sm["coupled_eta"], sm["coupled_bound"],
             sm["coupled_asserted"], sm["rho_max"], sm["over_cap"], sm["over_cap_eta"]))
    for q, name, e, b, rho in recs:
        if name == "coupled":
            print("   coupled q%d (%s, item list %d): rho %.2e eta %.2e bound %s"
                  % (q, ref.kinds[q], np.bincount(ref.train[1], minlength=ref.I)[ref.qi[q]], rho, e,
                     "%.2e" % b if b is not None else "-- (rho over the cap)"))
