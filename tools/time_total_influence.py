"""Time fia_total_influence against the route it replaces, on the same work.

The route it replaces is built from entry points that exist without it: fia_query_batch_x with
full outputs (rel_idx, influence), then a device index_add_ of influence by rel_idx into a
vector of n_train.  Both run on the synthetic ml-1m workload of bench.py (synth.ML1M, all
12,074 test ratings, k = 16) with the inverse HVPs x precomputed, so neither includes the solve.

Per figure: warm-up calls, then --steps calls each timed by its own pair of HIP events on the
stream (torch events); the median is reported, with the minimum and maximum beside it.  The
library's phase events split the new call into score (everything up to the train-row pass) and
topk (the merge).  Prints one JSON line per model.

    python tools/time_total_influence.py --model MF --steps 30 --warmup 5
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fia-kdd-19_amd"))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="MF", choices=["MF", "NCF"])
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--K", type=int, default=64, help="top-K of the extra fia_total_influence figure")
    args = ap.parse_args()

    import torch
    from influence import _lib, synth

    k = 16
    d = synth.make_dataset(synth.ML1M, seed=0)
    params = (synth.mf_params if args.model == "MF" else synth.ncf_params)(d["U"], d["I"], k, 0)
    tu, ti, tr = d["train"]
    qu_np, qi_np, _ = d["test"]
    order = np.lexsort((qu_np, qi_np))          # bench.py's (item-major) query order
    qu_np, qi_np = np.ascontiguousarray(qu_np[order]), np.ascontiguousarray(qi_np[order])
    U, I = d["U"], d["I"]
    dev = torch.device("cuda", 0)
    ctx = _lib.Context(0)
    tables = [torch.from_numpy(np.ascontiguousarray(params[n], np.float32)).to(dev) for n in params]
    ctx.set_params(_lib.FIA_MODEL_MF if args.model == "MF" else _lib.FIA_MODEL_NCF, k, U, I, tables, 1e-3, 1e-6)
    t_u, t_i, t_r = (torch.from_numpy(a).to(dev) for a in (tu, ti, tr))
    ctx.build_index(t_u, t_i, t_r, U, I)
    ctx.prepare()
    qu, qi = torch.from_numpy(qu_np).to(dev), torch.from_numpy(qi_np).to(dev)
    off, total_rel = ctx.count_related(qu, qi)
    Q, D, n = qu.numel(), ctx.num_params(), ctx.n_train
    rel = torch.empty(total_rel, dtype=torch.int32, device=dev)
    infl = torch.empty(total_rel, dtype=torch.float64, device=dev)
    x = torch.empty(Q * D, dtype=torch.float64, device=dev)
    ctx.query_batch(qu, qi, off, total_rel, rel, infl, x, 0, None, None, None)      # x, once

    base = torch.zeros(n, dtype=torch.float64, device=dev)
    total = torch.empty(n, dtype=torch.float64, device=dev)
    count = torch.empty(n, dtype=torch.int32, device=dev)
    tk_i = torch.empty(args.K, dtype=torch.int64, device=dev)
    tk_v = torch.empty(args.K, dtype=torch.float64, device=dev)

    def old_route():
        ctx.query_batch_x(qu, qi, off, total_rel, x, rel, infl, 0, None, None, None)
        base.zero_()
        base.index_add_(0, rel.long(), infl)

    def old_scatter_only():
        base.zero_()
        base.index_add_(0, rel.long(), infl)

    def new_call():
        ctx.total_influence(qu, qi, x, total, count)

    def new_call_topk():
        ctx.total_influence(qu, qi, x, total, count, args.K, tk_i, tk_v)

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize(dev)
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
        for a, b in ev:
            a.record()
            fn()
            b.record()
        torch.cuda.synchronize(dev)
        ms = sorted(a.elapsed_time(b) for a, b in ev)
        return dict(median_ms=ms[len(ms) // 2], min_ms=ms[0], max_ms=ms[-1])

    def phases(fn):
        out = {}
        for ph in ("score", "topk"):             # one phase at a time: each event pair costs stream time
            ctx.set_profiling(True, [ph])
            ctx.profile_read()
            for _ in range(args.steps):
                fn()
            torch.cuda.synchronize(dev)
            ms, cnt = ctx.profile_read()[ph]
            out[ph + "_ms"] = ms / max(cnt, 1)
        ctx.set_profiling(False)
        return out

    old_route()
    new_call()
    torch.cuda.synchronize(dev)
    a, b = base.cpu().numpy(), total.cpu().numpy()
    agree = float(np.abs(a - b).max() / np.abs(a).max())
    counts_equal = bool(np.array_equal(count.cpu().numpy(), np.bincount(rel.cpu().numpy(), minlength=n)))
    out = dict(model=args.model, k=k, queries=Q, n_train=int(n), total_rel=int(total_rel), steps=args.steps,
               warmup=args.warmup,
               old_route=timed(old_route), old_scatter_only=timed(old_scatter_only),
               total_influence=timed(new_call), total_influence_topk=timed(new_call_topk),
               total_influence_phases=phases(new_call), total_influence_topk_phases=phases(new_call_topk), K=args.K,
               max_rel_diff_vs_old_route=agree, count_equals_bincount=counts_equal)
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
