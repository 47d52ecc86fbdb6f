"""Time fia_score_candidates against the scoring phase of fia_query_batch_x on the same work.

For a bench.py config (ml1m-mf, yelp-ncf) and its query set (item-major order, as bench.py
runs it) the candidates are each query's own related rows (tu[rel], ti[rel], tr[rel]), so both
calls do the same arithmetic for the same ratings: fia_query_batch_x(full, K=0) with the benefit
of the per-list-position caches, fia_score_candidates from the parameter tables alone.

Per call: HIP-event time of the library's 'score' phase (fia_set_profiling, one phase at a time)
and the stream time of the whole call (torch events), warm-up first, then the mean over --steps.
Prints one JSON line per config.

    python tools/time_candidates.py --config ml1m-mf --steps 20 --warmup 3
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fia-kdd-19_amd"))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

HBM_PEAK_GBS = 8000.0


def gathered_bytes(model, k):
    """Bytes one candidate reads through its ids (table rows; cache-resident when the tables are
    small) and the 20 B it streams (two int32 ids, a float32 rating, a float64 result)."""
    rows = 2 * 4 * k if model == "MF" else 2 * 8 * k + 2 * 4 * k     # NCF: two l1 rows (fp64) + two GMF rows
    return 20, rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="ml1m-mf", choices=["ml1m-mf", "yelp-ncf"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()

    import torch
    import bench
    from influence import _lib

    cfg = bench.CONFIGS[args.config]
    d, params = bench.load_data(cfg)
    tu, ti, tr = d["train"]
    qu_np, qi_np, _ = d["test"]
    order = np.lexsort((qu_np, qi_np))
    qu_np, qi_np = np.ascontiguousarray(qu_np[order]), np.ascontiguousarray(qi_np[order])
    U, I, k = d["U"], d["I"], cfg["k"]
    dev = torch.device("cuda", 0)
    ctx = _lib.Context(0)
    tables = [torch.from_numpy(np.ascontiguousarray(params[n], np.float32)).to(dev) for n in params]
    ctx.set_params(_lib.FIA_MODEL_MF if cfg["model"] == "MF" else _lib.FIA_MODEL_NCF, k, U, I, tables, 1e-3, 1e-6)
    t_u, t_i, t_r = (torch.from_numpy(a).to(dev) for a in (tu, ti, tr))
    ctx.build_index(t_u, t_i, t_r, U, I)
    ctx.prepare()
    qu, qi = torch.from_numpy(qu_np).to(dev), torch.from_numpy(qi_np).to(dev)
    off, total = ctx.count_related(qu, qi)
    Q, D = qu.numel(), ctx.num_params()
    rel = torch.empty(total, dtype=torch.int32, device=dev)
    infl = torch.empty(total, dtype=torch.float64, device=dev)
    x = torch.empty(Q * D, dtype=torch.float64, device=dev)
    ctx.query_batch(qu, qi, off, total, rel, infl, x, 0, None, None, None)
    rows = rel.long()
    c_u, c_i, c_r = t_u[rows].contiguous(), t_i[rows].contiguous(), t_r[rows].contiguous()
    cand = torch.empty(total, dtype=torch.float64, device=dev)
    ctx.score_candidates(qu, qi, x, off, total, c_u, c_i, c_r, cand, 0, None, None)
    torch.cuda.synchronize(dev)
    a, b = infl.cpu().numpy(), cand.cpu().numpy()
    ok = np.isfinite(a)
    worst = float(np.abs(a[ok] - b[ok]).max() / np.abs(a[ok]).max())

    def run(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize(dev)
        ctx.set_profiling(True, ["score"])
        ctx.profile_read()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.steps):
            fn()
        e1.record()
        torch.cuda.synchronize(dev)
        ms, cnt = ctx.profile_read()["score"]
        ctx.set_profiling(False)
        return ms / max(cnt, 1), e0.elapsed_time(e1) / args.steps

    base_score, base_call = run(lambda: ctx.query_batch_x(qu, qi, off, total, x, rel, infl, 0, None, None, None))
    cand_score, cand_call = run(lambda: ctx.score_candidates(qu, qi, x, off, total, c_u, c_i, c_r, cand, 0, None,
                                                             None))
    stream, rows_b = gathered_bytes(cfg["model"], k)
    out = dict(config=args.config, model=cfg["model"], k=k, queries=Q, candidates=int(total), steps=args.steps,
               query_batch_x_score_ms=base_score, query_batch_x_call_ms=base_call,
               score_candidates_score_ms=cand_score, score_candidates_call_ms=cand_call,
               candidates_per_s=total / (cand_score * 1e-3),
               related_ratings_per_s_query_batch_x=total / (base_score * 1e-3),
               streamed_bytes_per_candidate=stream, gathered_row_bytes_per_candidate=rows_b,
               streamed_fraction_of_hbm_peak=stream * total / (cand_score * 1e-3) / (HBM_PEAK_GBS * 1e9),
               streamed_plus_gathered_fraction_of_hbm_peak=(stream + rows_b) * total / (cand_score * 1e-3) /
               (HBM_PEAK_GBS * 1e9),
               max_rel_diff_vs_query_batch=worst)
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
