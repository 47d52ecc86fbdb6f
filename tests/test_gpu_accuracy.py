"""The fp64 accuracy of the Gram, solve and scoring kernels across conditioning: every query's x
by its BACKWARD error against a longdouble restatement of its system, under a bound derived
from the arithmetic (Gram accumulation length, elimination growth, the NCF gradient chain), and
every related rating's influence against the longdouble scoring of the GPU's own x.  The
problems, the regimes, the reference and the derivations are tests/accuracy_problems.py;
tests/test_accuracy_cpu.py validates that yardstick without a GPU.

Per (configuration, regime) one context, one fia_prepare, one fia_query_batch (K = 1, x
requested), asserted in this order:
  1. related sets bit-exact against CsrExact;
  2. eta(x_gpu) <= bound for every asserted system (each side block of an uncoupled query; the
     full system of a coupled query whose growth rho <= 1e3);
  3. |influence - infl_ld(x_gpu)| <= the scoring bound for every related rating of every query;
  4. the query with n = 0 gives NaN x.
A coupled query above the rho cap is held to the suite's standard only (x within RTOL of the
oracle's np.linalg.solve x); its eta is printed beside the numpy LDL^T's.  MF k = 32, 64 repeat
`base` and `nodecay` with K = 2: scoring through k_score_grouped_mf instead of
k_score_mf_mfma.

A system over its bound is a finding in the kernel (Gram accumulation, reciprocal, elimination
or back solve), never a reason to widen the bound."""
import numpy as np
import pytest

import accuracy_problems as ap
from test_gpu_mfma_score import RawModel
from test_gpu_parity import RTOL, rel_err

pytestmark = pytest.mark.gpu

CASES = [(c, r, 1) for c in ap.CONFIGS for r in ap.REGIMES] + \
        [(c, r, 2) for c in (("MF", 32), ("MF", 64)) for r in ("base", "nodecay")]


def case_id(v):
    return ap.config_id(v) if isinstance(v, tuple) else "K%d" % v if isinstance(v, int) else None


@pytest.mark.parametrize("cfg,regime,K", CASES, ids=case_id)
def test_backward_error_and_scoring(cfg, regime, K):
    from oracle import fia_oracle as fo
    model, k = cfg
    ref = ap.reference(model, k, regime)
    lo = ap.lib_order(model, k)
    m = RawModel(model, k, ref.U, ref.I, ref.train, ref.params, wd=ref.wd, damping=ref.damping)
    res = m.batch(ref.qu, ref.qi, K)
    m.close()
    Q = ref.qu.size
    x_lib = res["x"][:, lo]

    # 1. related sets
    ex = fo.CsrExact(model, ref.params, k, ref.train[0], ref.train[1], ref.train[2], ref.wd, ref.damping)
    for q in range(Q):
        b, e = res["offsets"][q], res["offsets"][q + 1]
        assert np.array_equal(res["rel_idx"][b:e], ex.related(int(ref.qu[q]), int(ref.qi[q]))), q
        assert np.array_equal(res["rel_idx"][b:e], ref.related(int(ref.qu[q]), int(ref.qi[q]))), q

    # 2. backward error of x
    recs = ap.judge(ref, lambda q: x_lib[q])
    sm = ap.summary(recs)
    print("%s k=%d %s K=%d: side eta %.2e (bound %.2e, eta / bound %.1e) | coupled eta %.2e (bound %.2e, "
          "eta / bound %.1e, %d asserted) | rho max %.1e, %d over the cap"
          % (model, k, regime, K, sm["side_eta"], sm["side_bound"], sm["side_ratio"], sm["coupled_eta"],
             sm["coupled_bound"], sm["coupled_ratio"], sm["coupled_asserted"], sm["rho_max"], sm["over_cap"]))
    over = []
    for q, name, eta, bound, rho in recs:
        assert np.isfinite(x_lib[q]).all(), (model, k, regime, q)
        if bound is None:
            over.append((q, eta, rho))
            continue
        assert eta <= bound, (model, k, regime, q, ref.kinds[q], name, eta, bound, rho)
    for q, eta, rho in over:
        s = ref.system(q)
        H64, v64 = s["H"].astype(np.float64), s["v"].astype(np.float64)
        eta_np = ap.eta(s["H"], s["v"], ap.ldlt_solve(H64.copy(), v64.copy()))
        err = rel_err(x_lib[q], np.linalg.solve(H64, v64))
        print("   over the cap: q%d (%s) rho %.2e: eta gpu %.2e, eta numpy LDL^T %.2e, x vs np.linalg.solve %.2e"
              % (q, ref.kinds[q], rho, eta, eta_np, err))
        assert err < RTOL, (model, k, regime, q, err, eta, rho)

    # 3. scoring, with the GPU's own x
    worst = 0.0
    for q in range(Q):
        b, e = res["offsets"][q], res["offsets"][q + 1]
        if e == b:
            continue
        want, bound = ref.influence(q, x_lib[q])
        err = np.abs(res["influence"][b:e].astype(ap.LD) - want)
        worst = max(worst, float((err / bound).max()))
        j = int(np.argmax(err / bound))
        assert (err <= bound).all(), (model, k, regime, K, q, ref.kinds[q], j, float(err[j]), float(bound[j]))
    print("   scoring: largest |influence - infl_ld(x_gpu)| / bound %.1e" % worst)

    # 4. n = 0
    q0 = ref.kinds.index("none")
    assert res["offsets"][q0 + 1] == res["offsets"][q0] and np.isnan(res["x"][q0]).all()
    assert [q for q in range(Q) if np.isnan(res["x"][q]).any()] == [q0]
